// PLAID candidate generation from the compressed token store (include/sskd_amd.h, "Candidate generation").
//
// The compressed store of late.hip holds, per token, the id of its nearest centroid.  With an inverted file over those ids
// (list c = the rows that own a token of centroid c) the store retrieves by itself:
//   plaid_scores_kernel    S[c, t] = <centroid_c, q_t> for every query token of the batch, on v_mfma_f32_32x32x16_bf16;
//   plaid_probe_kernel     per query token the nprobe best centroids of every part of the centroid range, one lane per
//                          token, the list in registers;  plaid_probe_merge_kernel merges the parts;
//   plaid_union_kernel     the rows of the probed lists, OR-ed into a per-query bitmap;
//   plaid_compact_kernel   the bitmap AND the allow-mask, ranked by popcounts into an ascending row list;
//   plaid_interact_kernel  approx(q, r) = sum_i max_j S[cid_j, t_i] over ALL tokens of r, one wave per (query, candidate);
//   plaid_select_kernel    the best R by (approx descending, row ascending): radix select on a 64-bit key, rank-order sort.
// Everything after S is a function of S's bits: no step rounds but the sequential fp32 sum of the interaction.
#include "late_device.h"
#include "search_host.h"   // sskd::MAX_SHARD_ROWS: rows are int32 per index

namespace {

constexpr int P_NPROBE_MAX = SSKD_PLAID_NPROBE_MAX;   // 32
constexpr int P_PARTS_MAX = 64;                 // parts of the centroid range one token's probe search is cut into
constexpr int P_RANK_THREADS = 1024;
constexpr size_t WORKSPACE_BUDGET = (size_t)256 << 20;   // what the size query asks for at most (if one query fits)

// ------------------------------------------------------------------------------------------------ centroid scores
// The tile engine of late_device.h with one block: a workgroup of 4 waves serves one block of 32 query tokens, staged once
// in LDS; wave w walks centroid tiles of 32 rows.  Element (c, t) is the chain of 24 MFMAs over row c and row t alone, so
// its bits do not depend on what else the batch holds.  Tokens past T are zero rows, centroids past C re-read the last
// real row; neither is stored.
__global__ __launch_bounds__(L_THREADS) void plaid_scores_kernel(const bf16x8* __restrict__ q_tokens, int64_t T,
                                                                 const bf16x8* __restrict__ centroids, int C,
                                                                 float* __restrict__ S, int64_t ld) {
  __shared__ QueryFragments<1> qs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const int64_t t0 = (int64_t)blockIdx.y * 32;
  stage_query<1>(qs, q_tokens, t0, (int)(T - t0 < 32 ? T - t0 : 32));
  __syncthreads();
  const int tiles = (C + 31) >> 5;
  for (int ct = blockIdx.x * L_WAVES + wave; ct < tiles; ct += gridDim.x * L_WAVES) {
    const int c = min(ct * 32 + r32, C - 1);
    bf16x8 a[L_KSTEPS];
    load_row_fragments(a, centroids + (int64_t)c * L_ROW_VEC + h);
    const f32x16 acc = tile_product(a, qs[0], lane);
    // register r of lane l: centroid 32 ct + acc_row(r) + 4 (l >> 5), query token t0 + (l & 31): 128 contiguous bytes
    // per lane half and register
    if (t0 + r32 < T) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = ct * 32 + acc_row(r) + 4 * h;
        if (row < C) S[(int64_t)row * ld + t0 + r32] = acc[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ shared pieces
struct PlaidParams {
  const float* S;            // [C, ld]
  int64_t ld;
  const int64_t* q_lims;     // [nq + 1]
  int64_t n_q_tokens;
  const int32_t* cid;        // [n_tokens]
  const int64_t* tok_lims;   // [n_rows + 1]
  const int64_t* list_lims;  // [C + 1]
  const int32_t* list_rows;  // [n_list]
  const uint32_t* row_mask;  // NULL = all rows
  int64_t n_rows, n_tokens, n_list, id_offset;
  int C, nprobe, R, q0;      // q0: first query of this chunk
  int parts, span;           // probe search: parts of `span` centroids each
  int words;                 // ceil(n_rows / 32)
  // workspace of the chunk, indexed by the query's position ql in it
  float* part_s;             // [chunk][L_TQ_MAX][parts][nprobe]
  int32_t* part_c;           //   "
  int32_t* probes;           // [chunk][L_TQ_MAX][nprobe]
  uint32_t* bitmap;          // [chunk][words_pad]
  int32_t* rows;             // [chunk][rows_pad]   the candidates, ascending
  float* approx;             // [chunk][rows_pad]
  int32_t* count;            // [chunk]             |Cand(q)|
  int64_t words_pad, rows_pad;
  int64_t* cand_ids;         // [nq, R]
  float* cand_scores;        // [nq, R]
  int32_t* n_cand;           // [nq]
};

// the query's token range (late_device.h), at most L_TQ_MAX tokens of it
__device__ inline void query_range(const PlaidParams& p, int q, int64_t& q_begin, int& Tq) {
  int64_t tq;
  query_range(p.q_lims, p.n_q_tokens, q, q_begin, tq);
  Tq = (int)(tq < L_TQ_MAX ? tq : L_TQ_MAX);
}

// ------------------------------------------------------------------------------------------------ probes
// The project's per-lane register top-k: the lane's NP best so far, sorted, in registers.  A lane meets its centroids in
// ascending order, so among equal scores the earlier one stays ahead when a newcomer must be STRICTLY better to pass.
// (-inf, -1) is the empty slot: `v > -inf` is false for -inf and for NaN, so neither is ever picked.
template <int NP>
struct ProbeList {
  float s[NP];
  int c[NP];
  __device__ inline void clear() {
#pragma unroll
    for (int j = 0; j < NP; ++j) { s[j] = -INFINITY; c[j] = -1; }
  }
  __device__ inline void offer(float v, int id) {
    if (!(v > s[NP - 1])) return;
    s[NP - 1] = v;
    c[NP - 1] = id;
#pragma unroll
    for (int j = NP - 1; j > 0; --j) {
      if (s[j] > s[j - 1]) {
        const float ts = s[j]; s[j] = s[j - 1]; s[j - 1] = ts;
        const int tc = c[j]; c[j] = c[j - 1]; c[j - 1] = tc;
      }
    }
  }
};

// grid (ceil(Tq_pad * parts / 256), chunk): thread -> (part, token) with the token fastest, so that the lanes of a wave
// read consecutive floats of one row of S.  Part `part` covers centroids [part * span, (part + 1) * span).
template <int NP>
__global__ __launch_bounds__(L_THREADS) void plaid_probe_kernel(const PlaidParams p, int tq_pad) {
  const int ql = blockIdx.y, q = p.q0 + ql;
  int64_t q_begin;
  int Tq;
  query_range(p, q, q_begin, Tq);
  const int slot = blockIdx.x * L_THREADS + threadIdx.x;
  const int i = slot % tq_pad, part = slot / tq_pad;
  if (i >= Tq || part >= p.parts) return;
  ProbeList<NP> best;
  best.clear();
  const int c_begin = part * p.span, c_end = min(c_begin + p.span, p.C);
  const float* col = p.S + q_begin + i;
#pragma unroll 8
  for (int c = c_begin; c < c_end; ++c) best.offer(col[(int64_t)c * p.ld], c);
  const int64_t out = (((int64_t)ql * L_TQ_MAX + i) * p.parts + part) * p.nprobe;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (j < p.nprobe) {
      p.part_s[out + j] = best.s[j];
      p.part_c[out + j] = best.c[j];
    }
  }
}

// One thread per (query, token): nprobe rounds over the heads of the parts' sorted lists (a cursor per part in LDS).  The
// parts cover ascending centroid ranges, so the first part among equal heads holds the lowest centroid.
__global__ __launch_bounds__(64) void plaid_probe_merge_kernel(const PlaidParams p) {
  __shared__ uint8_t cursor[P_PARTS_MAX][64];
  const int ql = blockIdx.y, q = p.q0 + ql;
  int64_t q_begin;
  int Tq;
  query_range(p, q, q_begin, Tq);
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= L_TQ_MAX) return;
  int32_t* out = p.probes + ((int64_t)ql * L_TQ_MAX + i) * p.nprobe;
  if (i >= Tq) {
    for (int j = 0; j < p.nprobe; ++j) out[j] = -1;
    return;
  }
  for (int l = 0; l < p.parts; ++l) cursor[l][threadIdx.x] = 0;
  const int64_t base = ((int64_t)ql * L_TQ_MAX + i) * p.parts * p.nprobe;
  for (int j = 0; j < p.nprobe; ++j) {
    float bs = -INFINITY;
    int bc = -1, bl = -1;
    for (int l = 0; l < p.parts; ++l) {
      const int at = cursor[l][threadIdx.x];
      if (at >= p.nprobe) continue;
      const int c = p.part_c[base + (int64_t)l * p.nprobe + at];
      const float s = p.part_s[base + (int64_t)l * p.nprobe + at];
      if (c >= 0 && (bc < 0 || s > bs)) { bs = s; bc = c; bl = l; }
    }
    out[j] = bc;                      // -1 from here on: fewer than nprobe centroids have a score that can be picked
    if (bl >= 0) cursor[bl][threadIdx.x] += 1;
  }
}

// ------------------------------------------------------------------------------------------------ union
// One wave per (query, token, probe): the rows of the probed list are OR-ed into the query's bitmap.  A centroid probed
// by several tokens is walked once per token: the OR does not care.  list_lims is read clamped into [0, n_list] and a
// row outside [0, n_rows) is skipped, so a damaged list cannot write outside the bitmap.
__global__ __launch_bounds__(L_THREADS) void plaid_union_kernel(const PlaidParams p) {
  const int ql = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * L_WAVES + (threadIdx.x >> 6);
  if (slot >= L_TQ_MAX * p.nprobe) return;
  const int c = p.probes[(int64_t)ql * L_TQ_MAX * p.nprobe + slot];
  if (c < 0 || c >= p.C) return;
  int64_t lo = p.list_lims[c], hi = p.list_lims[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > p.n_list ? p.n_list : hi;
  uint32_t* bits = p.bitmap + (int64_t)ql * p.words_pad;
  for (int64_t at = lo + lane; at < hi; at += 64) {
    const int r = p.list_rows[at];
    if (r >= 0 && (int64_t)r < p.n_rows) atomicOr(&bits[r >> 5], 1u << (r & 31));
  }
}

// One workgroup per query walks the bitmap as row_mask_rank_kernel walks a mask, carrying the running count: the word is
// ANDed with the allow-mask, the bits at or past n_rows are dropped, and the set bits of word w become rows
// 32 w + bit at positions prefix(w) ..: the list ascends.
__global__ __launch_bounds__(P_RANK_THREADS) void plaid_compact_kernel(const PlaidParams p) {
  __shared__ uint32_t wave_total[P_RANK_THREADS / 64];
  const int ql = blockIdx.x, q = p.q0 + ql;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* bits = p.bitmap + (int64_t)ql * p.words_pad;
  int32_t* rows = p.rows + (int64_t)ql * p.rows_pad;
  const uint32_t last_keep = (p.n_rows & 31) ? (1u << (p.n_rows & 31)) - 1u : ~0u;
  uint32_t carry = 0;
  for (int base = 0; base < p.words; base += P_RANK_THREADS) {
    const int w = base + tid;
    uint32_t v = 0u;
    if (w < p.words) {
      v = bits[w];
      if (p.row_mask) v &= p.row_mask[w];
      if (w == p.words - 1) v &= last_keep;
    }
    const uint32_t mine = __popc(v);
    uint32_t incl = mine;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t below = __shfl_up(incl, o);
      if (lane >= o) incl += below;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < P_RANK_THREADS / 64; ++i) {
      const uint32_t x = wave_total[i];
      if (i < wave) before += x;
      total += x;
    }
    uint32_t at = carry + before + (incl - mine);
    while (v) {
      const int bit = __ffs((int)v) - 1;
      v &= v - 1u;
      rows[at++] = 32 * w + bit;
    }
    carry += total;
    __syncthreads();  // wave_total is rewritten by the next step
  }
  if (tid == 0) {
    p.count[ql] = (int32_t)carry;
    p.n_cand[q] = (int32_t)carry;
  }
}

// ------------------------------------------------------------------------------------------------ interaction
// One wave per (query, candidate); the waves of a query stride over its candidate list, so the work follows the list's
// length, not n_rows.  The wave reads 64 centroid ids of the document in one instruction; then, per PAIR of document
// tokens, lanes 0 .. 31 read the Tq contiguous floats of one row of S and lanes 32 .. 63 those of the next - one 128-byte
// line per lane half at Tq = 32 - eight pairs in flight.  Each lane keeps the running max of its (token half, query
// token); the halves meet through lane l ^ 32 and the query's tokens are summed in ascending order, sequentially, from
// +0.0f.  Lanes past the document's end repeat its last token (a repeated element does not change a max), lanes past Tq
// repeat the last query token and are not summed.  The max ignores NaN (fmaxf) and starts from -inf.
//   Which workgroup serves which query is chosen for the L2: workgroups are dealt to the 8 XCDs round-robin by their
// linear id, so workgroup id serves query 8 (id / 8 / per_query) + id % 8 as its worker id / 8 % per_query - the
// per_query workgroups of a query follow each other on ONE XCD, and that XCD's L2 holds the few slabs of S (C * Tq
// floats each) its resident workgroups gather from.  Placement is not a contract: another dealing is slower, not wrong.
// Fewer than 8 queries would leave XCDs idle that way: their workgroups are dealt query by query over the whole chip.
__global__ __launch_bounds__(L_THREADS) void plaid_interact_kernel(const PlaidParams p, int n_queries, int per_query) {
  int ql, worker;
  if (n_queries >= 8) {
    const int seq = blockIdx.x >> 3;
    ql = 8 * (seq / per_query) + (blockIdx.x & 7);
    worker = seq % per_query;
  } else {
    ql = blockIdx.x / per_query;
    worker = blockIdx.x % per_query;
  }
  if (ql >= n_queries) return;
  const int q = p.q0 + ql;
  const int lane = threadIdx.x & 63, r32 = lane & 31, h = lane >> 5;
  int64_t q_begin;
  int Tq;
  query_range(p, q, q_begin, Tq);
  const int n = p.count[ql];
  const int32_t* rows = p.rows + (int64_t)ql * p.rows_pad;
  float* approx = p.approx + (int64_t)ql * p.rows_pad;
  const int nb = (Tq + 31) >> 5;
  for (int ci = worker * L_WAVES + (threadIdx.x >> 6); ci < n; ci += per_query * L_WAVES) {
    const int64_t row = rows[ci];
    int64_t lo = 0, hi = 0;
    if (row >= 0 && row < p.n_rows) { lo = p.tok_lims[row]; hi = p.tok_lims[row + 1]; }
    if (lo < 0 || hi > p.n_tokens || hi < lo) hi = lo = 0;
    const int64_t td = hi - lo;
    float score = -INFINITY;                 // a row without tokens: every max is empty
    if (td > 0 && Tq > 0) {
      score = 0.f;
      for (int b = 0; b < nb; ++b) {
        const int left = Tq - 32 * b;       // query tokens of this block
        const float* col = p.S + q_begin + 32 * b + (r32 < left ? r32 : left - 1);
        float m = -INFINITY;
        for (int64_t t0 = 0; t0 < td; t0 += 64) {
          const int cnt = (int)(td - t0 < 64 ? td - t0 : 64);
          const int mine = p.cid[lo + t0 + (lane < cnt ? lane : cnt - 1)];
          const int cen = min(max(mine, 0), p.C - 1);   // a corrupt store scores garbage and cannot fault
          // eight pairs per step, all loaded before the first max waits; a pair past the end repeats the last token
          const int pairs = (cnt + 1) >> 1;
          for (int pr0 = 0; pr0 < pairs; pr0 += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int c = __shfl(cen, min(2 * (pr0 + u) + h, 63));
              v[u] = col[(int64_t)c * p.ld];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);
          }
        }
        m = fmaxf(m, __shfl_xor(m, 32));
        const int cnt_q = left < 32 ? left : 32;
        for (int i = 0; i < cnt_q; ++i) score += __shfl(m, i);
      }
    }
    if (lane == 0) approx[ci] = score;
  }
}

// ------------------------------------------------------------------------------------------------ selection
// key = (order-preserving image of approx) << 32 | ~row: the unsigned order of the keys is (approx descending, row
// ascending) read from the top, it is total, and the result does not depend on how the waves interleave.  NaN and -inf
// have no key.
__device__ inline bool select_key(float a, int32_t row, uint64_t& key) {
  if (!(a > -INFINITY)) return false;
  const uint32_t u = __float_as_uint(a);
  const uint32_t f = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  key = ((uint64_t)f << 32) | (uint32_t)(~(uint32_t)row);
  return true;
}

struct SelectShared {
  int hist[256];
  int sel_digit, sel_above, sel_count;
  int out_count, valid;
  uint64_t win[L_R_MAX];
};

// One workgroup per query.  Radix select, 8 bits per pass from the top (the scheme of bm25.hip's select, on one 64-bit
// word and up to 1 024 winners), then the winners are ordered by counting, for each, the winners ahead of it.
__global__ __launch_bounds__(L_THREADS) void plaid_select_kernel(const PlaidParams p) {
  __shared__ SelectShared sh;
  const int ql = blockIdx.x, q = p.q0 + ql;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = p.count[ql];
  const int32_t* rows = p.rows + (int64_t)ql * p.rows_pad;
  const float* approx = p.approx + (int64_t)ql * p.rows_pad;
  int64_t* oi = p.cand_ids + (int64_t)q * p.R;
  float* os = p.cand_scores + (int64_t)q * p.R;
  if (tid == 0) { sh.valid = 0; sh.out_count = 0; }
  __syncthreads();
  int local = 0;
  for (int i = tid; i < n; i += L_THREADS) local += approx[i] > -INFINITY ? 1 : 0;
  local = wave_sum(local);
  if (lane == 0 && local) atomicAdd(&sh.valid, local);
  __syncthreads();
  const int kk = min(p.R, sh.valid);          // (uniform)
  for (int i = kk + tid; i < p.R; i += L_THREADS) { oi[i] = -1; os[i] = -INFINITY; }
  if (kk <= 0) return;
  uint64_t thr = 0;
  int need = kk;
  for (int pass = 0; pass < 8; ++pass) {
    sh.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += L_THREADS) {
      uint64_t key;
      if (!select_key(approx[i], rows[i], key)) continue;
      if (pass > 0 && (key >> (64 - 8 * pass)) != (thr >> (64 - 8 * pass))) continue;
      atomicAdd(&sh.hist[(int)((key >> (56 - 8 * pass)) & 255u)], 1);
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
    thr |= (uint64_t)digit << (56 - 8 * pass);
    if (count == need) break;  // (uniform) everything under this prefix is wanted
  }
  // the winners: every key >= threshold, exactly kk of them
  for (int i = tid; i < n; i += L_THREADS) {
    uint64_t key;
    if (select_key(approx[i], rows[i], key) && key >= thr) {
      const int at = atomicAdd(&sh.out_count, 1);
      if (at < L_R_MAX) sh.win[at] = key;
    }
  }
  __syncthreads();
  const int won = min(sh.out_count, kk);
  for (int e = tid; e < won; e += L_THREADS) {
    const uint64_t key = sh.win[e];
    int rank = 0;
    for (int j = 0; j < won; ++j) rank += sh.win[j] > key ? 1 : 0;   // (every lane reads the same slot: broadcast)
    const uint32_t f = (uint32_t)(key >> 32);
    oi[rank] = (int64_t)(~(uint32_t)key) + p.id_offset;
    os[rank] = __uint_as_float((f & 0x80000000u) ? (f & 0x7FFFFFFFu) : ~f);
  }
}

// ------------------------------------------------------------------------------------------------ host
struct Plan {
  int words;
  int64_t words_pad, rows_pad;
  int parts, span, tq_pad;
  size_t per_query;
};

inline int64_t pad64(int64_t n) { return (n + 63) & ~(int64_t)63; }

// the chunk's carve: the size query and the launch code run this very function
struct Carve {
  float* part_s;
  int32_t *part_c, *probes, *rows, *count;
  uint32_t* bitmap;
  float* approx;
  size_t bytes;
};

inline Carve carve(void* base, const Plan& pl, int chunk, int nprobe) {
  sskd::Carver ws(base);
  Carve c;
  const size_t n = (size_t)chunk;
  c.part_s = ws.take<float>(n * L_TQ_MAX * P_PARTS_MAX * nprobe);
  c.part_c = ws.take<int32_t>(n * L_TQ_MAX * P_PARTS_MAX * nprobe);
  c.probes = ws.take<int32_t>(n * L_TQ_MAX * nprobe);
  c.bitmap = ws.take<uint32_t>(n * (size_t)pl.words_pad);
  c.rows = ws.take<int32_t>(n * (size_t)pl.rows_pad);
  c.approx = ws.take<float>(n * (size_t)pl.rows_pad);
  c.count = ws.take<int32_t>(n);
  c.bytes = ws.bytes();
  return c;
}

inline bool shape_ok(int nq, int max_tq, int C, int64_t n_rows, int nprobe, int R) {
  return nq >= 1 && max_tq >= 1 && max_tq <= L_TQ_MAX && C >= 1 && C <= L_C_MAX && n_rows >= 0 &&
         n_rows < sskd::MAX_SHARD_ROWS && nprobe >= 1 && nprobe <= P_NPROBE_MAX && nprobe <= C && R >= 1 && R <= L_R_MAX;
}

inline Plan make_plan(int chunk, int max_tq, int C, int64_t n_rows, int nprobe) {
  Plan pl;
  pl.words = (int)((n_rows + 31) >> 5);
  pl.words_pad = pad64(pl.words + 1);
  pl.rows_pad = pad64(n_rows + 1);
  pl.tq_pad = 32 * ((max_tq + 31) / 32);
  // parts: enough threads to fill the chip for a single query, few when there are many queries; a part holds at least 32
  // centroids and at least nprobe of them
  int64_t parts = sskd::ceil_div(512 * (int64_t)sskd::cu_count(), (int64_t)chunk * pl.tq_pad);
  const int64_t most = sskd::ceil_div(C, nprobe > 32 ? nprobe : 32);
  if (parts > most) parts = most;
  if (parts > P_PARTS_MAX) parts = P_PARTS_MAX;
  if (parts < 1) parts = 1;
  pl.span = (int)sskd::ceil_div(C, parts);
  pl.parts = (int)sskd::ceil_div(C, pl.span);
  pl.per_query = carve(nullptr, pl, 1, nprobe).bytes;
  return pl;
}

// bytes of one query's worth: depends on (n_rows, nprobe) alone, never on the device
inline size_t per_query_bytes(int64_t n_rows, int nprobe) {
  Plan pl;
  pl.words = (int)((n_rows + 31) >> 5);
  pl.words_pad = pad64(pl.words + 1);
  pl.rows_pad = pad64(n_rows + 1);
  return carve(nullptr, pl, 1, nprobe).bytes;
}

// the largest chunk whose carve fits `bytes` (every array's start is rounded to 256 bytes: at most 7 x 256 beyond the sum)
inline int chunk_that_fits(size_t bytes, int64_t n_rows, int nprobe, int nq) {
  const size_t one = per_query_bytes(n_rows, nprobe);
  size_t fit = bytes / one;
  if (fit > 65535) fit = 65535;   // grid.y
  if (fit > (size_t)nq) fit = (size_t)nq;
  return (int)fit;
}

// workgroups of the interaction per query: about 8 per compute unit in all for a few queries, and never fewer than 64 -
// the 256 workgroups resident on an XCD then gather from the slabs of S of 4 queries, which its L2 holds at 4 096
// centroids - but no more than there are candidates to give each wave one
inline int64_t interact_per_query(int chunk, int64_t n_rows) {
  int64_t g = sskd::ceil_div(8 * (int64_t)sskd::cu_count(), chunk);
  if (g < 64) g = 64;
  const int64_t most = sskd::ceil_div(n_rows > 0 ? n_rows : 1, L_WAVES);
  return g > most ? most : g;
}

template <int NP>
void launch_probe(const PlaidParams& p, const Plan& pl, int n, hipStream_t st) {
  const unsigned gx = (unsigned)sskd::ceil_div((int64_t)pl.tq_pad * pl.parts, L_THREADS);
  hipLaunchKernelGGL(plaid_probe_kernel<NP>, dim3(gx, (unsigned)n), dim3(L_THREADS), 0, st, p, pl.tq_pad);
}

}  // namespace

extern "C" {

int sskd_plaid_centroid_scores(const void* d_q_tokens, int64_t n_q_tokens, const void* d_centroids, int C, float* d_S,
                               int64_t ld, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_q_tokens >= 0 && n_q_tokens <= (int64_t)65535 * 32, "plaid_centroid_scores: n_q_tokens=%lld outside [0, %lld]",
               (long long)n_q_tokens, (long long)65535 * 32);
  SSKD_REQUIRE(C >= 1 && C <= L_C_MAX, "plaid_centroid_scores: C=%d outside [1, %d]", C, L_C_MAX);
  SSKD_REQUIRE(ld >= n_q_tokens, "plaid_centroid_scores: ld=%lld < n_q_tokens=%lld", (long long)ld, (long long)n_q_tokens);
  if (n_q_tokens == 0) return SSKD_OK;
  SSKD_REQUIRE(d_q_tokens && d_centroids && d_S, "plaid_centroid_scores: null pointer");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_centroids) && reinterpret_cast<uintptr_t>(d_S) % 4 == 0,
               "plaid_centroid_scores: query tokens and centroids must be 16-byte aligned");
  const int64_t gy = sskd::ceil_div(n_q_tokens, 32);
  const int64_t groups = sskd::ceil_div(sskd::ceil_div(C, 32), L_WAVES);
  int64_t gx = sskd::ceil_div(8 * (int64_t)sskd::cu_count(), gy);   // about 8 workgroups per compute unit in all
  if (gx > groups) gx = groups;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(plaid_scores_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(L_THREADS), 0, sskd::as_stream(stream),
                     static_cast<const bf16x8*>(d_q_tokens), n_q_tokens, static_cast<const bf16x8*>(d_centroids), C, d_S, ld);
  return sskd::check_launch("plaid_scores_kernel");
}

size_t sskd_plaid_candidates_workspace_bytes(int nq, int64_t n_rows, int nprobe) {
  if (nq < 1 || n_rows < 0 || n_rows >= sskd::MAX_SHARD_ROWS || nprobe < 1 || nprobe > P_NPROBE_MAX) return 0;
  const size_t one = per_query_bytes(n_rows, nprobe);
  // min(nq queries, max(budget, one query)): monotone in nq
  const size_t all = one * (size_t)nq;
  const size_t cap = one > WORKSPACE_BUDGET ? one : WORKSPACE_BUDGET;
  return all < cap ? all : cap;
}

int sskd_plaid_candidates_plan(int nq, int max_tq, int C, int64_t n_rows, int nprobe, int R, size_t workspace_bytes,
                               size_t* per_query_bytes_out, int* queries_per_chunk, int* probe_parts,
                               int* interact_workgroups) {
  SSKD_REQUIRE(shape_ok(nq, max_tq, C, n_rows, nprobe, R),
               "plaid_candidates_plan: needs nq >= 1, 1 <= Tq <= %d, 1 <= C <= %d, 1 <= nprobe <= min(C, %d), 1 <= R <= %d", L_TQ_MAX,
               L_C_MAX, P_NPROBE_MAX, L_R_MAX);
  const size_t have = workspace_bytes ? workspace_bytes : sskd_plaid_candidates_workspace_bytes(nq, n_rows, nprobe);
  const int chunk = chunk_that_fits(have, n_rows, nprobe, nq);
  SSKD_REQUIRE(chunk >= 1, "plaid_candidates_plan: a workspace of %zu B does not hold one query (%zu B)", have,
               per_query_bytes(n_rows, nprobe));
  const Plan pl = make_plan(chunk, max_tq, C, n_rows, nprobe);
  if (per_query_bytes_out) *per_query_bytes_out = pl.per_query;
  if (queries_per_chunk) *queries_per_chunk = chunk;
  if (probe_parts) *probe_parts = pl.parts;
  if (interact_workgroups) *interact_workgroups = (int)interact_per_query(chunk, n_rows);
  return SSKD_OK;
}

int sskd_plaid_candidates(const float* d_S, int64_t ld, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int C,
                          const int32_t* d_cid, const int64_t* d_tok_lims, int64_t n_rows, int64_t n_tokens,
                          const int64_t* d_list_lims, const int32_t* d_list_rows, int64_t n_list, const uint32_t* d_row_mask,
                          int nprobe, int R, int64_t id_offset, int64_t* d_cand_ids, float* d_cand_scores, int32_t* d_n_cand,
                          void* d_workspace, size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0, "plaid_candidates: nq < 0");
  SSKD_REQUIRE(C >= 1 && C <= L_C_MAX, "plaid_candidates: C=%d outside [1, %d]", C, L_C_MAX);
  SSKD_REQUIRE(nprobe >= 1 && nprobe <= P_NPROBE_MAX && nprobe <= C, "plaid_candidates: nprobe=%d outside [1, min(C=%d, %d)]",
               nprobe, C, P_NPROBE_MAX);
  SSKD_REQUIRE(R >= 1 && R <= L_R_MAX, "plaid_candidates: R=%d outside [1, %d]", R, L_R_MAX);
  SSKD_REQUIRE(n_rows >= 0 && n_tokens >= 0 && id_offset >= 0, "plaid_candidates: n_rows, n_tokens and id_offset must be >= 0");
  if (int rc = sskd::require_shard_rows("plaid_candidates", n_rows)) return rc;
  SSKD_REQUIRE(n_list >= 0 && n_list <= n_tokens,
               "plaid_candidates: the centroid lists hold %lld rows, a store of %lld tokens has at most that many (centroid, row) pairs",
               (long long)n_list, (long long)n_tokens);
  if (nq == 0) return SSKD_OK;
  const int max_tq = check_query_lims("plaid_candidates", q_lims, nq);
  if (max_tq < 0) return SSKD_ERR_INVALID;
  SSKD_REQUIRE(ld >= q_lims[nq], "plaid_candidates: ld=%lld < the batch's %lld query tokens", (long long)ld, (long long)q_lims[nq]);
  SSKD_REQUIRE(d_S && d_q_lims && d_list_lims && d_cand_ids && d_cand_scores && d_n_cand, "plaid_candidates: null pointer");
  SSKD_REQUIRE(n_list == 0 || d_list_rows, "plaid_candidates: null list rows");
  const bool store = d_cid && d_tok_lims;
  SSKD_REQUIRE(n_rows == 0 || store || n_tokens == 0, "plaid_candidates: null token store");
  const size_t one = per_query_bytes(n_rows, nprobe);
  if (int rc = sskd::require_workspace("plaid_candidates", d_workspace, workspace_bytes, one)) return rc;
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % 256 == 0, "plaid_candidates: workspace must be 256-byte aligned");
  const int chunk = chunk_that_fits(workspace_bytes, n_rows, nprobe, nq);
  const Plan pl = make_plan(chunk, max_tq, C, n_rows, nprobe);
  const Carve cv = carve(d_workspace, pl, chunk, nprobe);

  PlaidParams p{};
  p.S = d_S;
  p.ld = ld;
  p.q_lims = d_q_lims;
  p.n_q_tokens = q_lims[nq];
  p.cid = d_cid;
  p.tok_lims = d_tok_lims;
  p.list_lims = d_list_lims;
  p.list_rows = d_list_rows;
  p.row_mask = d_row_mask;
  p.n_rows = store ? n_rows : 0;
  p.n_tokens = store ? n_tokens : 0;
  p.n_list = n_list;
  p.id_offset = id_offset;
  p.C = C;
  p.nprobe = nprobe;
  p.R = R;
  p.parts = pl.parts;
  p.span = pl.span;
  p.words = store ? pl.words : 0;
  p.part_s = cv.part_s;
  p.part_c = cv.part_c;
  p.probes = cv.probes;
  p.bitmap = cv.bitmap;
  p.rows = cv.rows;
  p.approx = cv.approx;
  p.count = cv.count;
  p.words_pad = pl.words_pad;
  p.rows_pad = pl.rows_pad;
  p.cand_ids = d_cand_ids;
  p.cand_scores = d_cand_scores;
  p.n_cand = d_n_cand;
  hipStream_t st = sskd::as_stream(stream);
  const int64_t ig = interact_per_query(chunk, n_rows);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = nq - q0 < chunk ? nq - q0 : chunk;
    // (the chunks reuse the workspace: stream order keeps a chunk's selection ahead of the next chunk's probes)
    p.q0 = q0;
    if (hipMemsetAsync(cv.bitmap, 0, (size_t)n * (size_t)pl.words_pad * sizeof(uint32_t), st) != hipSuccess)
      return sskd::fail(SSKD_ERR_HIP, "plaid_candidates: cannot clear the bitmaps");
    if (nprobe <= 1) launch_probe<1>(p, pl, n, st);
    else if (nprobe <= 2) launch_probe<2>(p, pl, n, st);
    else if (nprobe <= 4) launch_probe<4>(p, pl, n, st);
    else if (nprobe <= 8) launch_probe<8>(p, pl, n, st);
    else if (nprobe <= 16) launch_probe<16>(p, pl, n, st);
    else launch_probe<32>(p, pl, n, st);
    if (int rc = sskd::check_launch("plaid_probe_kernel")) return rc;
    hipLaunchKernelGGL(plaid_probe_merge_kernel, dim3(L_TQ_MAX / 64, (unsigned)n), dim3(64), 0, st, p);
    if (int rc = sskd::check_launch("plaid_probe_merge_kernel")) return rc;
    hipLaunchKernelGGL(plaid_union_kernel, dim3((unsigned)sskd::ceil_div(L_TQ_MAX * nprobe, L_WAVES), (unsigned)n), dim3(L_THREADS), 0,
                       st, p);
    if (int rc = sskd::check_launch("plaid_union_kernel")) return rc;
    hipLaunchKernelGGL(plaid_compact_kernel, dim3((unsigned)n), dim3(P_RANK_THREADS), 0, st, p);
    if (int rc = sskd::check_launch("plaid_compact_kernel")) return rc;
    hipLaunchKernelGGL(plaid_interact_kernel, dim3((unsigned)((n >= 8 ? 8 * sskd::ceil_div(n, 8) : n) * ig)), dim3(L_THREADS), 0, st, p, n, (int)ig);
    if (int rc = sskd::check_launch("plaid_interact_kernel")) return rc;
    hipLaunchKernelGGL(plaid_select_kernel, dim3((unsigned)n), dim3(L_THREADS), 0, st, p);
    if (int rc = sskd::check_launch("plaid_select_kernel")) return rc;
  }
  return SSKD_OK;
}

}  // extern "C"
