// select_bit_check.cpp -- the host form of csrc/bb_device.h's select_bit against the six-level routine it replaced.
//
// A stand-alone program (its own main; nothing is loaded into Python): tests/test_select_bit_native.py compiles
// it for the host only, once plain and once with -fsanitize=undefined (the shift and extract widths), and runs
// it.  Every k in 0..69 -- past any popcount, so the out-of-contract answers are held equal too: the quota pass
// calls select_bit in dummy lanes -- over N random words (argv[1], default 2^20) of each of five density
// classes, over 0 and over the 64 single-bit words.  Exit status 1 at the first mismatch.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../block-blast-ai---reinforcement-learning-agent_amd/csrc/bb_device.h"

// The routine as it stood before the prefix-popcount search, verbatim but for the name of the population count
// (__popc is a device function).
static inline uint32_t popc_ref(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
static int select_bit_six_level(uint64_t x, uint32_t k) {
  int pos = 0;
  uint32_t c = popc_ref((uint32_t)x);
  if (k >= c) { k -= c; x >>= 32; pos += 32; }
  c = popc_ref((uint32_t)x & 0xFFFFu);
  if (k >= c) { k -= c; x >>= 16; pos += 16; }
  c = popc_ref((uint32_t)x & 0xFFu);
  if (k >= c) { k -= c; x >>= 8; pos += 8; }
  c = popc_ref((uint32_t)x & 0xFu);
  if (k >= c) { k -= c; x >>= 4; pos += 4; }
  c = popc_ref((uint32_t)x & 0x3u);
  if (k >= c) { k -= c; x >>= 2; pos += 2; }
  c = (uint32_t)x & 1u;
  if (k >= c) { pos += 1; }
  return pos;
}

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next64() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

static const char* const kClass[5] = {"uniform", "and2", "and4", "or3", "ones>>r"};
static uint64_t word_of(Rng& r, int cls) {
  switch (cls) {
    case 0: return r.next64();
    case 1: return r.next64() & r.next64();
    case 2: return r.next64() & r.next64() & r.next64() & r.next64();
    case 3: return r.next64() | r.next64() | r.next64();
    default: return ~0ull >> (r.next64() & 63u);
  }
}

static std::atomic<long> checked{0};
static std::atomic<bool> failed{false};
static bool same(uint64_t x, const char* what) {
  for (uint32_t k = 0; k < 70; ++k) {
    const int got = bb::select_bit(x, k), want = select_bit_six_level(x, k);
    if (got != want) {
      std::printf("MISMATCH (%s) x=%016llx k=%u: select_bit %d, six-level %d\n", what, (unsigned long long)x, k, got, want);
      return false;
    }
  }
  return true;
}

// The random part is cut into chunks, each a stream of its own (the same words whatever the thread count), so
// that the 350M pairs take the test seconds, not tens of them.
constexpr int kChunks = 8;
static void run_chunks(std::atomic<int>* next, long n) {
  for (int c; (c = next->fetch_add(1)) < 5 * kChunks && !failed.load();) {
    const int cls = c / kChunks, part = c % kChunks;
    Rng r{0x243F6A8885A308D3ull * (uint64_t)(c + 1)};
    for (long i = n * part / kChunks; i < n * (part + 1) / kChunks; ++i)
      if (!same(word_of(r, cls), kClass[cls])) {
        failed.store(true);
        return;
      }
    checked.fetch_add(70 * (n * (part + 1) / kChunks - n * part / kChunks));
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : (1L << 20);
  if (!same(0ull, "zero")) return 1;
  for (int b = 0; b < 64; ++b)
    if (!same(1ull << b, "single bit")) return 1;
  checked += 70 * 65;
  {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (unsigned q = 0; q < nt; ++q) pool.emplace_back(run_chunks, &next, n);
    for (auto& th : pool) th.join();
    if (failed.load()) return 1;
  }
  // in contract the answer is the k-th set bit: spot-check the meaning, not only the agreement
  Rng r{1};
  for (int i = 0; i < 4096; ++i) {
    const uint64_t x = word_of(r, i % 5);
    uint32_t k = 0;
    for (int b = 0; b < 64; ++b)
      if ((x >> b) & 1ull) {
        if (bb::select_bit(x, k) != b) {
          std::printf("MISMATCH x=%016llx k=%u: select_bit %d, bit %d\n", (unsigned long long)x, k, bb::select_bit(x, k), b);
          return 1;
        }
        ++k;
      }
  }
  std::printf("select_bit equals the six-level form: %ld (x, k) pairs, %ld words per class\n", checked.load(), n);
  return 0;
}
