#!/usr/bin/env python3
"""Diagnostics (not product): SHA-256 digests of every output buffer of the three fused losses and of
bb_masked_sample on a fixed list of seeded cases, for comparing two builds bit for bit (BBVEC_LIB selects the
library, runtime/lib.py).

    python tools/loss_bits.py --out profiles/lossrows/bits_branch.json

Cases: bb_{ppo,distill,guided}_loss_{forward,backward,fused}, f32 and bf16, B = 1, 5, 67, 259, 16,389; rows cycle
through 1, ~10% and 192 legal actions; distill and guided at tau 0 and 50 with an empty-M row and a row whose q is
all INT64_MIN (the PPO kernel gets the same rows without them), guided also without q and once with coefs_dev;
bb_masked_sample sampled from given uniforms, by Philox, deterministic and with action_in at n = 259.  Inputs come
from numpy generators, so two runs hash the same inputs.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"), REPO]

import torch  # noqa: E402

INT64_MIN = np.iinfo(np.int64).min
SIZES = (1, 5, 67, 259, 4 * 4096 + 5)
CLIP, COEFS = 0.2, (1.0, 0.5, 0.01, 0.3)


def rows(B, special):
    """Seeded rows: logits, values, mask bool [B, 192], actions in the mask, old_logp around the row's own log-prob,
    adv (every fourth 0), ret, q (INT64_MIN outside the mask and on ~5% inside).  ``special``: row 0 gets an empty
    mask and row 1 a q of INT64_MIN, as far as B allows."""
    rng = np.random.default_rng(4000 + B)
    logits = (rng.standard_normal((B, 192)) * 2.0).astype(np.float32)
    kind = np.arange(B) % 3
    M = np.where(kind[:, None] == 2, True, (rng.random((B, 192)) < 0.1) & (kind[:, None] == 1))
    first = rng.integers(192, size=B)
    M[np.arange(B), first] = True
    q = rng.integers(-400, 400, (B, 192)).astype(np.int64)
    stale = M & (rng.random((B, 192)) < 0.05)
    stale[np.arange(B), first] = False
    q[~M | stale] = INT64_MIN
    actions = np.array([rng.choice(np.flatnonzero(m)) for m in M], np.int64)
    x = np.where(M, logits.astype(np.float64), -np.inf)
    logp = x - x.max(1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))
    old = (logp[np.arange(B), actions] + (rng.random(B) - 0.5) * 0.8).astype(np.float32)
    old[::5] = logp[np.arange(B), actions][::5].astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    adv[3::4] = 0.0
    values = rng.standard_normal(B).astype(np.float32)
    ret = (values + rng.standard_normal(B) * 0.7).astype(np.float32)
    if special and B > 1:
        M[0] = False
        q[1] = INT64_MIN
    bits = (M.reshape(B, 3, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)
    return dict(logits=logits, values=values, mask=M.astype(np.float32), mask_bits=bits.view(np.int64),
                actions=actions, old_logp=old, adv=adv, ret=ret, q=q)


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def loss_case(name, form, t, nstats, fields, dev, has_dvalues=True):
    """One raw call of bb_<name>_loss_<form> on the device tensors t -> {buffer: digest}."""
    from runtime import kernels as K
    from runtime import lib as L

    lib, B = L.load(), t["logits"].shape[0]
    outs = {}
    if form in ("forward", "fused"):
        nbytes = getattr(lib, f"bb_{name}_loss_workspace_bytes")(B)
        outs.update(ws=torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev),
                    cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                    stats=torch.zeros(nstats, dtype=torch.float32, device=dev),
                    loss=torch.zeros(1, dtype=torch.float32, device=dev))
    if form in ("backward", "fused"):
        outs.update(grad_loss=torch.tensor([0.75], dtype=torch.float32, device=dev),
                    dlogits=torch.zeros_like(t["logits"]))
        if has_dvalues:
            outs["dvalues"] = torch.zeros_like(t["values"])
    cls = {"ppo": L.PpoLossArgs, "distill": L.DistillLossArgs, "guided": L.GuidedLossArgs}[name]
    a = cls(B=B, bf16=int(t["logits"].dtype == torch.bfloat16), **fields,
            **{k: v.data_ptr() for k, v in outs.items()})
    call = f"bb_{name}_loss_{form}"
    L.check(getattr(lib, call)(C.byref(a), K._s(dev)), call)
    torch.cuda.synchronize(dev)
    return {k: digest(outs[k]) for k in ("stats", "loss", "cnt", "dlogits", "dvalues") if k in outs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bits.py runs the kernels on the HIP device: none is visible")
    from runtime import kernels as K
    from runtime import lib as L

    dev = torch.device("cuda", 0)
    res = {}
    for B in SIZES:
        for bf16 in (False, True):
            dt = "bf16" if bf16 else "f32"
            for special in (False, True):
                t = {k: torch.from_numpy(v).to(dev) for k, v in rows(B, special).items()}
                if bf16:
                    t["logits"], t["values"] = t["logits"].bfloat16(), t["values"].bfloat16()
                p = {k: v.data_ptr() for k, v in t.items()}
                row = {k: p[k] for k in ("actions", "old_logp", "adv", "ret")}
                for form in ("forward", "backward", "fused"):
                    if not special:  # the PPO kernel has no rule for an empty row
                        f = dict(logits=p["logits"], values=p["values"], mask=p["mask"], clip=CLIP,
                                 value_coef=COEFS[1], entropy_coef=COEFS[2], **row)
                        res[f"ppo-{form}-{dt}-B{B}"] = loss_case("ppo", form, t, 6, f, dev)
                        continue
                    for tau in (0.0, 50.0):
                        f = dict(logits=p["logits"], mask_bits=p["mask_bits"], q=p["q"], tau=tau)
                        res[f"distill-{form}-{dt}-B{B}-tau{tau:g}"] = loss_case("distill", form, t, 6, f, dev, False)
                        for with_q in (True, False):
                            f = dict(logits=p["logits"], values=p["values"], mask_bits=p["mask_bits"], clip=CLIP,
                                     policy_coef=COEFS[0], value_coef=COEFS[1], entropy_coef=COEFS[2],
                                     distill_coef=COEFS[3] if with_q else 0.0, tau=tau, **row)
                            if with_q:
                                f["q"] = p["q"]
                            res[f"guided-{form}-{dt}-B{B}-tau{tau:g}-{'q' if with_q else 'noq'}"] = \
                                loss_case("guided", form, t, 12, f, dev)
    t = {k: torch.from_numpy(v).to(dev) for k, v in rows(259, True).items()}
    cdev = torch.tensor([0.7, 0.4, 0.03, 0.6, 20.0], dtype=torch.float32, device=dev)
    f = dict(logits=t["logits"].data_ptr(), values=t["values"].data_ptr(), mask_bits=t["mask_bits"].data_ptr(),
             q=t["q"].data_ptr(), clip=CLIP, coefs_dev=cdev.data_ptr(),
             **{k: t[k].data_ptr() for k in ("actions", "old_logp", "adv", "ret")})
    res["guided-fused-f32-B259-coefs_dev"] = loss_case("guided", "fused", t, 12, f, dev)
    t = {k: torch.from_numpy(v).to(dev) for k, v in rows(259, False).items()}  # no empty row: its outputs are NaN
    u = torch.from_numpy(np.random.default_rng(9).random(259).astype(np.float32)).to(dev)
    for name, kw in (("uniform", dict(uniform=u)), ("philox", dict(seed=11, step=3, env_offset=5)),
                     ("deterministic", dict(deterministic=True)), ("action_in", dict(action_in=t["actions"]))):
        act, logp, ent = K.masked_sample(t["logits"], t["mask_bits"], **kw)
        torch.cuda.synchronize(dev)
        res[f"masked_sample-{name}-n259"] = dict(action=digest(act), logp=digest(logp), entropy=digest(ent))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1, sort_keys=True) + "\n")  # digests alone: two builds' files compare with cmp
    print(json.dumps({"cases": len(res), "build_id": L.build_id(), "out": args.out}))


if __name__ == "__main__":
    main()
