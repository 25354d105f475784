// Workgroup radix select over 96-bit keys in rank order (internal: not installed).  bm25.hip ranks rows with it
// (score, then row), expand.hip ranks expansion terms (weight, then term id).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sskd {
namespace radix {

constexpr int SELECT_THREADS = 256;   // the workgroup that calls select_sorted
constexpr int SELECT_K_MAX = 256;     // winners it can hand out

// fp64 -> uint64 whose unsigned order is the order of the doubles (no NaN reaches here: idf and w are finite)
__device__ inline uint64_t score_key(double s) {
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double key_score(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

struct SelectShared {
  int hist[256];
  int sel_digit, sel_above, sel_count;
  int out_count;
  uint64_t win_hi[SELECT_K_MAX];
  uint32_t win_lo[SELECT_K_MAX];
};

// The `kk` largest of n elements under the 96-bit key (hi, lo), handed to emit(rank, hi, lo) with rank 0 = largest.
// load(i, hi, lo) returns false for an empty slot.  Keys are distinct (lo carries the row), so the order is total and
// the result does not depend on how the waves interleave.  Radix select, 8 bits per pass from the top: a histogram of
// the digit among the elements that still match the prefix, the bin that holds the kk-th largest, next digit.  It stops
// as soon as the bin is needed whole.  LO_DIGITS = bytes of `lo`, from the top, that can differ.  Called by the whole
// workgroup with uniform n and kk (it holds barriers); 0 <= kk <= min(SELECT_K_MAX, valid elements).
template <int LO_DIGITS, class Load, class Emit>
__device__ inline void select_sorted(SelectShared& sh, int n, int kk, Load load, Emit emit) {
  constexpr int THREADS = SELECT_THREADS;
  const int tid = threadIdx.x, lane = tid & 63;
  if (kk <= 0) return;  // (uniform)
  uint64_t thr_hi = 0;
  uint32_t thr_lo = 0;
  int need = kk;
  if (tid == 0) sh.out_count = 0;
  for (int p = 0; p < 8 + LO_DIGITS; ++p) {
    sh.hist[tid] = 0;
    __syncthreads();
    for (int base = tid - lane; base < n; base += THREADS) {   // every lane of a wave stays in the loop (ballots)
      const int i = base + lane;
      uint64_t hi = 0;
      uint32_t lo = 0;
      bool match = i < n && load(i, hi, lo);
      int digit;
      if (p < 8) {
        match = match && (p == 0 || (hi >> (64 - 8 * p)) == (thr_hi >> (64 - 8 * p)));
        digit = (int)((hi >> (56 - 8 * p)) & 255u);
      } else {
        const int r = p - 8;
        match = match && hi == thr_hi && (r == 0 || (lo >> (32 - 8 * r)) == (thr_lo >> (32 - 8 * r)));
        digit = (int)((lo >> (24 - 8 * r)) & 255u);
      }
      const unsigned long long m = __ballot(match);
      if (m) {
        // a wave whose matching lanes share one digit (a tile of untouched +0.0 rows) adds once, not 64 times
        const int leader = __ffsll((long long)m) - 1;
        const int first = __shfl(digit, leader);
        if (__ballot(match && digit == first) == m) {
          if (lane == leader) atomicAdd(&sh.hist[first], __popcll(m));
        } else if (match) {
          atomicAdd(&sh.hist[digit], 1);
        }
      }
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: lane l owns bins 4l .. 4l + 3; suffix sums across the lanes
      const int h0 = sh.hist[4 * lane], h1 = sh.hist[4 * lane + 1], h2 = sh.hist[4 * lane + 2], h3 = sh.hist[4 * lane + 3];
      const int mine = h0 + h1 + h2 + h3;
      int suffix = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_down(suffix, o);
        if (lane + o < 64) suffix += v;
      }
      const int a3 = suffix - mine, a2 = a3 + h3, a1 = a2 + h2, a0 = a1 + h1;
      int d = -1, above = 0, count = 0;
      if (a3 < need && need <= a3 + h3) { d = 3; above = a3; count = h3; }
      else if (a2 < need && need <= a2 + h2) { d = 2; above = a2; count = h2; }
      else if (a1 < need && need <= a1 + h1) { d = 1; above = a1; count = h1; }
      else if (a0 < need && need <= a0 + h0) { d = 0; above = a0; count = h0; }
      if (d >= 0) {
        sh.sel_digit = 4 * lane + d;
        sh.sel_above = above;
        sh.sel_count = count;
      }
    }
    __syncthreads();
    const int digit = sh.sel_digit, count = sh.sel_count;
    need -= sh.sel_above;
    if (p < 8) thr_hi |= (uint64_t)digit << (56 - 8 * p);
    else thr_lo |= (uint32_t)digit << (24 - 8 * (p - 8));
    if (count == need) break;  // (uniform) everything under this prefix is wanted
  }
  // the winners: every key >= threshold, exactly kk of them
  for (int i = tid; i < n; i += THREADS) {
    uint64_t hi = 0;
    uint32_t lo = 0;
    if (load(i, hi, lo) && (hi > thr_hi || (hi == thr_hi && lo >= thr_lo))) {
      const int at = atomicAdd(&sh.out_count, 1);
      if (at < SELECT_K_MAX) {
        sh.win_hi[at] = hi;
        sh.win_lo[at] = lo;
      }
    }
  }
  __syncthreads();
  const int won = min(sh.out_count, min(kk, SELECT_K_MAX));
  if (tid < won) {
    const uint64_t hi = sh.win_hi[tid];
    const uint32_t lo = sh.win_lo[tid];
    int rank = 0;
    for (int j = 0; j < won; ++j) {   // (every lane reads the same slot: broadcast)
      const uint64_t oh = sh.win_hi[j];
      const uint32_t ol = sh.win_lo[j];
      rank += (oh > hi || (oh == hi && ol > lo)) ? 1 : 0;
    }
    if (rank < kk) emit(rank, hi, lo);
  }
}

}  // namespace radix
}  // namespace sskd
