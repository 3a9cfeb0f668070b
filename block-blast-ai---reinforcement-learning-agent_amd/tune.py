#!/usr/bin/env python3
"""CLI: python tune.py --agent plan --depth 3 --population 64 --games 8 --moves 300 --generations 30 --seed 1 \\
                       --output weights.json --log tune.jsonl   (cross-entropy method over the search weights)
        python tune.py --compare weights.json --games 100 --moves 3000 --seed 42   (against the defaults)
        --fitness survival [--horizon N] prices survival by the refill census; --compare ... --census adds its columns"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

from evaluation.tune import main  # noqa: E402

if __name__ == "__main__":
    main()
