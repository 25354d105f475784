// The walk over a padded ranking (internal: not installed).  Every kernel that post-processes a first stage's result reads
// a `[nq][width]` ranking of (score, id) the same way, one wave, 64 ranks per round: the first id -1 (every search's
// padding) ENDS the ranking, that rank and all behind it do not count; an id outside [0, n_rows) in front of the end is
// SKIPPED and the walk goes on; the kernel's own predicate decides among the rest; the survivors are PACKED in rank order.
// This is part of the C ABI's contract (tests/*_cases.py restate it, tests/ranking_walk_cases.py holds the rankings that
// tell the variants apart).  Per kernel:
//   kernel                 ends on     lanes behind   differs from the common walk in
//   compact_candidates     -1          cut            nothing                                                   (mmr.hip)
//   prf_rocchio_kernel     -1          cut            walks the first fb_docs ranks only                     (expand.hip)
//   prf_rm3_kernel         -1          cut            also drops score == 0.0 and masked rows; stops at fb_docs survivors
//   hybrid_fuse_kernel     -1          cut            wave 0 dense, wave 1 BM25; a survivor keeps its slot `at` and takes
//                                                     only its 1-based rank from the pack; BM25 as rm3        (hybrid.hip)
//   mine_select_kernel     any id < 0  cut            ANY negative id ends the ranking, not -1 alone            (mine.hip)
//   group_collapse_kernel  any id < 0  NOT cut        a negative id only marks the ranking exhausted (the same call's exact
//                                                     search wrote it: the padding is a suffix); groups are de-duplicated
//                                                     between step and pack, count clamped to k            (grouped.hip)
//   rank_denoise_kernel    -1          (no step)      workgroup-wide: the length is an atomicMin over id == -1, ids outside
//                                                     the store are NOT skipped (empty sets, they stay in the output), the
//                                                     pack goes over four waves: block_walk_pack (as graph.hip's pick
//                                                     of the next parents)                                  (denoise.hip)
// The two rules are compile-time parameters of the step; loop bound, extra predicates and stores stay with the caller.
// No floating point; the wave forms use no LDS and no barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace {

enum class WalkEnd { MinusOne, AnyNegative };

// The step.  `inside`: the lane's position is inside the list; `id`: what it loaded there.  Returns whether the lane holds
// a row of [0, n_rows) in front of the end; sets the wave-uniform `ended` once an end id was met.
template <WalkEnd END = WalkEnd::MinusOne, bool CUT_BEHIND_END = true>
__device__ __forceinline__ bool walk_step(bool inside, int64_t id, int64_t n_rows, int lane, bool& ended) {
  const unsigned long long pad = __ballot(inside && (END == WalkEnd::AnyNegative ? id < 0 : id == -1));
  bool alive = inside && id >= 0 && id < n_rows;
  if (pad) {
    ended = true;
    if (CUT_BEHIND_END && lane > __ffsll((long long)pad) - 1) alive = false;
  }
  return alive;
}

__device__ __forceinline__ int walk_lanes_ahead(unsigned long long surv, int lane) {
  return __popcll(surv & ((1ull << lane) - 1ull));
}

// The pack.  Returns the lane's 0-based place among the survivors so far (meaningful where `alive`) and advances the
// wave-uniform `count` by this round's survivors.
__device__ __forceinline__ int walk_pack(bool alive, int lane, int& count) {
  const unsigned long long surv = __ballot(alive);
  const int pos = count + walk_lanes_ahead(surv, lane);
  count += __popcll(surv);
  return pos;
}

// The pack over the WAVES waves of a workgroup, one thread per position: returns the thread's place among this round's
// survivors, `total` = how many there are.  One barrier inside; the caller puts one before s_count[WAVES] is used again.
template <int WAVES>
__device__ __forceinline__ int block_walk_pack(bool alive, int lane, int wave, int* s_count, int& total) {
  const unsigned long long surv = __ballot(alive);
  if (lane == 0) s_count[wave] = __popcll(surv);
  __syncthreads();
  int ahead = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) ahead += s_count[w];
    total += s_count[w];
  }
  return ahead + walk_lanes_ahead(surv, lane);
}

}  // namespace
