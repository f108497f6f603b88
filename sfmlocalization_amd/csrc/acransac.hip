// K3 / K5 of the query-localisation path for gfx950 (K4, which runs between them: k4_matchset.hip).
//
//   K3  k_fmatrix_filter     per surviving (view, query) pair: AC-RANSAC with the 7-point solver
//                            [reference: hulo::geometricMatch -> GeometricFilter_FMatrix_AC, MatchUtils.cpp:372-420]
//   K5  k_p3p_*              SfM_Localizer::Localize: AC-RANSAC with Kneip P3P on K^-1-normalised points,
//                            then KRt_From_P                                    [localization.cpp:504-509,544-547]
//
// AC-RANSAC is sequential by definition (the first meaningful model redirects sampling to its inliers and
// cuts the iteration budget to the reserved 10 %).  The kernels keep those semantics exactly and get their
// parallelism from speculation: hypotheses whose samples come from the CURRENT index set are evaluated in
// parallel, one workgroup per hypothesis (residuals -> LDS -> bitonic sort -> NFA scan -> block argmin), and
// a selection step replays the sequential rule over them in iteration order, discarding everything after
// the first hypothesis that changes the index set.  Samples come from a counter-based generator
// (Philox4x32-10 keyed by seed/stage/stream/iteration), so iteration i draws the same sample no matter
// which round evaluates it.  All arithmetic is f64, in the operation order of geom_device.h.
#include <string.h>
#include <float.h>

#include <type_traits>

#include "ransac_device.h"

namespace sfmloc {

namespace {

// Diagnostic build only (make EXTRA=-DSFMLOC_STAMPS OUT=../lib/libsfmloc_hip_stamps.so, tools/k35_stamps.py): thread 0
// of a workgroup records wall_clock64() (100 MHz) at stage boundaries of K3 and K5.  Compiles to nothing otherwise.
#ifdef SFMLOC_STAMPS
__device__ unsigned long long g_stamps_p3p[16 * 256 * 8];  // [round][hypothesis][point]
__device__ unsigned long long g_stamps_sel[16 * 8];        // [round][point]
__device__ unsigned long long g_stamps_f[256 * 64];        // [workgroup][event]: tag << 48 | time
#define STAMP_P3P(rnd, b, k)                                                                      \
  do {                                                                                            \
    if (threadIdx.x == 0 && (rnd) < 16 && (b) < 256) g_stamps_p3p[(((rnd)*256) + (b)) * 8 + (k)] = wall_clock64(); \
  } while (0)
#define STAMP_SEL(rnd, k)                                                              \
  do {                                                                                 \
    if (threadIdx.x == 0 && (rnd) < 16) g_stamps_sel[(rnd)*8 + (k)] = wall_clock64(); \
  } while (0)
#define STAMP_F_DECL int stamp_f_n = 0
#define STAMP_F(tag)                                                                                         \
  do {                                                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < 256 && stamp_f_n < 64)                                              \
      g_stamps_f[blockIdx.x * 64 + stamp_f_n++] = ((unsigned long long)(tag) << 48) | (wall_clock64() & 0xFFFFFFFFFFFFull); \
  } while (0)
#else
#define STAMP_P3P(rnd, b, k) do {} while (0)
#define STAMP_SEL(rnd, k) do {} while (0)
#define STAMP_F_DECL do {} while (0)
#define STAMP_F(tag) do {} while (0)
#endif

// ---------------------------------------------------------------------------------------------------
// block-wide helpers (256 threads)
// ---------------------------------------------------------------------------------------------------
// (pair_less, bitonic_sort, NfaBest, best_nfa_block, next_pow2: ransac_device.h -- relpose.hip uses them too)
// bestNFA over one wave's sorted segment; every lane of the wave returns the result
__device__ NfaBest best_nfa_wave(const uint64_t *key, int n, int s, double max_thr, double logalpha0, double mult,
                                 double loge0, const float *logc_n, const float *logc_k) {
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
  for (int kk = s + 1 + (int)(threadIdx.x & 63); kk <= n; kk += 64) {
    const double ek = u2d(key[kk - 1]);
    if (ek <= max_thr) {
      const double logalpha = logalpha0 + mult * det_log10(ek + (double)FLT_EPSILON);
      const double nfa = loge0 + logalpha * (double)(kk - s) + (double)logc_n[kk] + (double)logc_k[kk];
      if (nfa < lb) {
        lb = nfa;
        lk = kk;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(lb, off, 64);
    const int ok = __shfl_xor(lk, off, 64);
    if (ob < lb || (ob == lb && ok < lk)) {
      lb = ob;
      lk = ok;
    }
  }
  return NfaBest{lb, lk};
}

// ---------------------------------------------------------------------------------------------------
// register-resident wave sort: 64*E (key, idx) pairs, element e = r*64 + lane in register r.  The same bitonic
// network as bitonic_sort: strides >= 64 are compare-exchanges between two registers of one lane, strides < 64
// exchange with lane ^ j through ds_bpermute.  The order by (key, idx) is total, so any correct sort gives the
// same array.
// ---------------------------------------------------------------------------------------------------
template <int E>
__device__ __forceinline__ void wave_sort_regs(uint64_t (&key)[E], uint32_t (&idx)[E]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 2; k <= 64 * E; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
        const int jr = j >> 6;
#pragma unroll
        for (int r = 0; r < E; ++r) {
          if ((r & jr) == 0) {
            const int r2 = r | jr;
            const bool up = ((r << 6) & k) == 0;  // k >= 128: only the register index decides the direction
            const bool a_gt_b = pair_less(key[r2], idx[r2], key[r], idx[r]);
            if (a_gt_b == up) {
              const uint64_t tk = key[r];
              key[r] = key[r2];
              key[r2] = tk;
              const uint32_t ti = idx[r];
              idx[r] = idx[r2];
              idx[r2] = ti;
            }
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < E; ++r) {
          const uint64_t ok = __shfl_xor(key[r], j, 64);
          const uint32_t oi = __shfl_xor(idx[r], j, 64);
          const bool up = ((((r << 6) | lane) & k) == 0);
          const bool want_min = (((lane & j) == 0) == up);  // lower position of an ascending pair, or upper of a descending one
          if (pair_less(ok, oi, key[r], idx[r]) == want_min) {
            key[r] = ok;
            idx[r] = oi;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The same sort without LDS round trips (wave_sort_regs spends most of its time waiting for ds_bpermute: 33 dependent
// exchange stages for 256 elements).  Two changes:
//  * the element index rides in the low kPackBits bits of the 64-bit key, so a compare-exchange is one 64-bit compare
//    and two selects.  The 10 bits it displaces are the last bits of the residual's mantissa; they are parked in LDS
//    (`low`, one u32 per element, private to the wave) and put back after the sort.  Two keys that agree in everything
//    BUT those bits are ordered by index instead of by value; if that was wrong the restored keys do not ascend, which
//    is checked, and such a wave sorts again with wave_sort_regs.  The result is therefore always the order by
//    (key, idx) of the exact sort.
//  * lane ^ j exchanges are DPP moves (j = 1, 2, 4, 8) and gfx950's v_permlane16_swap / v_permlane32_swap (j = 16,
//    32); which lanes keep the minimum at a stage is a compile-time lane mask, applied with s_xor + v_cndmask.
// ---------------------------------------------------------------------------------------------------
constexpr int kPackBits = 10;  // 64 * 16 elements at most
constexpr uint64_t kPackMask = (1ull << kPackBits) - 1;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_perm(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);  // every lane is written: no `old` operand
}
// the value lane ^ J holds
template <int J>
__device__ __forceinline__ uint32_t lane_xor_u32(uint32_t v, bool odd_half) {
  if constexpr (J == 1) return dpp_perm<0xB1>(v);   // quad_perm:[1,0,3,2]
  if constexpr (J == 2) return dpp_perm<0x4E>(v);   // quad_perm:[2,3,0,1]
  if constexpr (J == 4) {                           // banks 0, 2 read lane + 4 (row_shl:4), banks 1, 3 lane - 4 (row_shr:4)
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x104, 0xF, 0x5, false);  // (banks 1, 3 are written next)
    return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)v, 0x114, 0xF, 0xA, false);
  }
  if constexpr (J == 8) return dpp_perm<0x128>(v);  // row_ror:8
  if constexpr (J == 16) {  // rows 1, 3 of the first operand <-> rows 0, 2 of the second
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return odd_half ? r[0] : r[1];
  }
  if constexpr (J == 32) {  // upper half of the first operand <-> lower half of the second
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return odd_half ? r[0] : r[1];
  }
  return v;
}
// lane bit set in m -> b, else a (m is wave-uniform: an SGPR pair)
__device__ __forceinline__ uint32_t select_by_mask(uint32_t a, uint32_t b, uint64_t m) {
  uint32_t r;
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
  return r;
}
// lanes l of register r that keep the smaller key at stage (k, j < 64) of the ascending bitonic network
constexpr uint64_t want_min_mask(int k, int j, int r) {
  uint64_t m = 0;
  for (int l = 0; l < 64; ++l) {
    const bool up = ((((r << 6) | l) & k) == 0);
    if (((l & j) == 0) == up) m |= 1ull << l;
  }
  return m;
}

template <int E, int K, int J>
__device__ __forceinline__ void packed_stage(uint64_t (&key)[E], int lane) {
  if constexpr (J >= 64) {
    constexpr int jr = J >> 6;
#pragma unroll
    for (int r = 0; r < E; ++r) {
      if ((r & jr) == 0) {
        const int r2 = r | jr;
        const bool up = ((r << 6) & K) == 0;
        const uint64_t a = key[r], b = key[r2];
        const bool swap = (a > b) == up;
        key[r] = swap ? b : a;
        key[r2] = swap ? a : b;
      }
    }
  } else {
    const bool odd_half = (lane & J) != 0;
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const uint32_t lo = (uint32_t)key[r], hi = (uint32_t)(key[r] >> 32);
      const uint32_t olo = lane_xor_u32<J>(lo, odd_half), ohi = lane_xor_u32<J>(hi, odd_half);
      const uint64_t o = ((uint64_t)ohi << 32) | olo;
      // take the partner's key where (partner < mine) == (this lane keeps the minimum)
      const uint64_t less = __builtin_amdgcn_ballot_w64(o < key[r]);
      const uint64_t take = ~(less ^ want_min_mask(K, J, r));
      key[r] = ((uint64_t)select_by_mask(hi, ohi, take) << 32) | select_by_mask(lo, olo, take);
    }
  }
}
template <int E, int K, int J>
__device__ __forceinline__ void packed_merge(uint64_t (&key)[E], int lane) {
  packed_stage<E, K, J>(key, lane);
  if constexpr (J > 1) packed_merge<E, K, (J >> 1)>(key, lane);
}
template <int E, int K>
__device__ __forceinline__ void packed_network(uint64_t (&key)[E], int lane) {
  if constexpr (K > 2) packed_network<E, (K >> 1)>(key, lane);
  packed_merge<E, K, (K >> 1)>(key, lane);
}

// key[r] / idx[r]: element r*64 + lane on entry (idx is overwritten), sorted position r*64 + lane on return;
// low: 64*E u32 of LDS owned by this wave (free on return).
template <int E>
__device__ __forceinline__ void wave_sort_fast(uint64_t (&key)[E], uint32_t (&idx)[E], uint32_t *low) {
  const int lane = threadIdx.x & 63;
  constexpr uint64_t kMask = E > 16 ? ((1ull << (kPackBits + 1)) - 1) : kPackMask;  // (the index of 64 E elements)
  static_assert(E <= 32, "the packed index holds 11 bits at most");
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const uint32_t p = (uint32_t)((r << 6) + lane);
    low[p] = (uint32_t)(key[r] & kMask);
    key[r] = (key[r] & ~kMask) | p;
  }
  packed_network<E, 64 * E>(key, lane);
#pragma unroll
  for (int r = 0; r < E; ++r) {
    idx[r] = (uint32_t)(key[r] & kMask);
    key[r] = (key[r] & ~kMask) | low[idx[r]];
  }
  // Keys that agree above the packed bits were ordered by index; that is the exact order unless their displaced bits
  // descend somewhere, i.e. unless the restored keys are not ascending.  (Equal keys -- the +inf residuals of a
  // degenerate model, the padding -- are in index order, which is the exact order.)
  bool ambiguous = false;
  uint64_t prev_last = 0ull;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    uint64_t before = __shfl_up(key[r], 1, 64);
    if (lane == 0) before = prev_last;
    if (before > key[r]) ambiguous = true;
    if (r + 1 < E) prev_last = __shfl(key[r], 63, 64);
  }
  if (__builtin_amdgcn_ballot_w64(ambiguous) != 0ull) wave_sort_regs<E>(key, idx);  // any order is a valid input
}

// bestNFA over the sorted registers of wave_sort_regs (position r*64 + lane holds e_{position+1}); same
// candidates, same per-lane visiting order and same reduction as best_nfa_wave
// the two table entries of sorted position r*64 + lane (k = position + 1), fetched ahead of the sort
template <int E>
__device__ __forceinline__ void nfa_tables_fetch(float (&cn)[E], float (&ck)[E], int n, const float *logc_n,
                                                 const float *logc_k) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int kk = (r << 6) + lane + 1;
    cn[r] = kk <= n ? logc_n[kk] : 0.0f;
    ck[r] = kk <= n ? logc_k[kk] : 0.0f;
  }
}
// wave_reduce_nfa: the same first-minimum reduction for both forms below
__device__ __forceinline__ NfaBest wave_reduce_nfa(double lb, int lk);

// K5's form (one wave per SIMD, latency-bound): the logarithms of all E positions first, branch-free, so that the E
// dependent chains interleave (values of positions that are not candidates are computed and dropped); table entries
// fetched ahead of the sort
template <int E>
__device__ __forceinline__ NfaBest best_nfa_regs_ilp(const uint64_t (&key)[E], int n, int s, double max_thr,
                                                     double logalpha0, double mult, double loge0, const float (&cn)[E],
                                                     const float (&ck)[E]) {
  const int lane = threadIdx.x & 63;
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
  double l10[E];
#pragma unroll
  for (int r = 0; r < E; ++r) l10[r] = det_log10_inline(u2d(key[r]) + (double)FLT_EPSILON);
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int kk = (r << 6) + lane + 1;
    if (kk > s && kk <= n) {
      const double ek = u2d(key[r]);
      if (ek <= max_thr) {
        const double logalpha = logalpha0 + mult * l10[r];
        const double nfa = loge0 + logalpha * (double)(kk - s) + (double)cn[r] + (double)ck[r];
        if (nfa < lb) {
          lb = nfa;
          lk = kk;
        }
      }
    }
  }
  return wave_reduce_nfa(lb, lk);
}

// K3's form (sixteen waves share a compute unit, issue-bound: fewer instructions and registers matter, latency does not)
template <int E>
__device__ __forceinline__ NfaBest best_nfa_regs(const uint64_t (&key)[E], int n, int s, double max_thr,
                                                 double logalpha0, double mult, double loge0, const float *logc_n,
                                                 const float *logc_k) {
  const int lane = threadIdx.x & 63;
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int kk = (r << 6) + lane + 1;
    if (kk > s && kk <= n) {
      const double ek = u2d(key[r]);
      if (ek <= max_thr) {
        const double logalpha = logalpha0 + mult * det_log10(ek + (double)FLT_EPSILON);
        const double nfa = loge0 + logalpha * (double)(kk - s) + (double)logc_n[kk] + (double)logc_k[kk];
        if (nfa < lb) {
          lb = nfa;
          lk = kk;
        }
      }
    }
  }
  return wave_reduce_nfa(lb, lk);
}
__device__ __forceinline__ NfaBest wave_reduce_nfa(double lb, int lk) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(lb, off, 64);
    const int ok = __shfl_xor(lk, off, 64);
    if (ob < lb || (ob == lb && ok < lk)) {
      lb = ob;
      lk = ok;
    }
  }
  return NfaBest{lb, lk};
}

// the key at sorted position pos (every lane returns it)
template <int E>
__device__ __forceinline__ uint64_t sorted_key_at(const uint64_t (&key)[E], int pos) {
  uint64_t v = 0;
#pragma unroll
  for (int r = 0; r < E; ++r)
    if ((pos >> 6) == r) v = key[r];
  return __shfl(v, pos & 63, 64);
}

// ---------------------------------------------------------------------------------------------------
// K3: F-matrix AC-RANSAC, one workgroup per selected view
// ---------------------------------------------------------------------------------------------------
constexpr int kFPre = 64;     // hypotheses solved speculatively per batch while sampling is still uniform

// (a write-through store: see "A round's results go from the workgroup that computed them ..." at K5)
template <typename T>
__device__ __forceinline__ void store_through(T *p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a workgroup of k_fmatrix_fast's wide form delivers for its iteration of the first batch: the models and their
// (NFA, inlier count)
struct K3Spec {
  double models[27];
  double nfa[3];
  int k[3];
  int nm;
};
struct FFilterArgs {
  const uint32_t *view_sel;
  uint32_t n_sel;
  const uint32_t *view_off, *view_id, *view_wh;
  const uint32_t *put_count, *match_i, *match_key;
  const float2 *map_kpt, *q_kpt6;
  uint32_t qw, qh;
  double precision;
  int n_iter;
  uint64_t seed;
  int min_putative;
  const double *L10;
  uint32_t *geo_count, *geo_idx;
  double *geo_model;  // [view][10]: the winning F (normalised frame) and its errorMax, for guided matching; or null
  uint32_t *large_count, *large_list;  // views with more than kFMaxM matches, queued for k_fmatrix_large (or null)
  int *status;
  int skip_le;  // k_fmatrix_filter leaves views with at most this many putative matches to k_fmatrix_fast
  int fast_min;  // k_fmatrix_fast<W, M> takes the views with fast_min < matches <= M
  MergeMaskedArgs merge;  // enabled: k_fmatrix_fast first builds its view's putative list (K2 left to it)
  K3Spec *spec;           // wide form: [view slot][kF2Batch] results of the first batch; per view slot the arrivals
  unsigned int *spec_arrive;
};
// How the list reaches a kernel.  As kernel arguments it is 280 bytes, and a gang launch -- the members' lists side by
// side in the 4 KB argument segment -- held 14 of them: a session of 32 queries went out as 14 + 14 + 4, three launches one
// after the other for each of K3's forms.  Most of the list never changes for a context (the map's tables, the context's
// own buffers, the parameters): that part lives on the device (FFilterStatic, written when it changes -- in practice
// once), the kernels get a pointer to it and what does change per launch (84 bytes: 32 members a launch), and put the list
// together again first thing.
struct FFilterStatic {
  const uint32_t *view_off, *view_id, *view_wh;
  const uint32_t *put_count, *match_i, *match_key;
  const float2 *map_kpt;
  double precision;
  int n_iter;
  uint64_t seed;
  const double *L10;
  uint32_t *geo_count, *geo_idx;
  double *geo_model;
  uint32_t *large_count, *large_list;
  int *status;
  MergeMaskedArgs merge;  // (enabled, view_sel, view_widx0: per launch, below)
};
struct FFilterArgsPacked {
  const FFilterStatic *st;
  const uint32_t *view_sel;
  const float2 *q_kpt6;
  const uint32_t *merge_view_sel, *merge_view_widx0;
  K3Spec *spec;
  unsigned int *spec_arrive;
  uint32_t n_sel, qw, qh;
  int min_putative, skip_le, fast_min, merge_enabled;
};
__device__ __forceinline__ FFilterArgs ffilter_expand(const FFilterArgsPacked &P) {
  const FFilterStatic &T = *P.st;
  FFilterArgs A;
  A.view_sel = P.view_sel;
  A.n_sel = P.n_sel;
  A.view_off = T.view_off;
  A.view_id = T.view_id;
  A.view_wh = T.view_wh;
  A.put_count = T.put_count;
  A.match_i = T.match_i;
  A.match_key = T.match_key;
  A.map_kpt = T.map_kpt;
  A.q_kpt6 = P.q_kpt6;
  A.qw = P.qw;
  A.qh = P.qh;
  A.precision = T.precision;
  A.n_iter = T.n_iter;
  A.seed = T.seed;
  A.min_putative = P.min_putative;
  A.L10 = T.L10;
  A.geo_count = T.geo_count;
  A.geo_idx = T.geo_idx;
  A.geo_model = T.geo_model;
  A.large_count = T.large_count;
  A.large_list = T.large_list;
  A.status = T.status;
  A.skip_le = P.skip_le;
  A.fast_min = P.fast_min;
  A.merge = T.merge;
  A.merge.enabled = P.merge_enabled;
  A.merge.view_sel = P.merge_view_sel;
  A.merge.view_widx0 = P.merge_view_widx0;
  A.spec = P.spec;
  A.spec_arrive = P.spec_arrive;
  return A;
}

// small per-view state of the block-wide form (always in LDS)
struct FSmall {
  double pre_models[kFPre][27];
  int pre_nm[kFPre];
  double cur_models[27];
  int cur_nm;
  double best_model[9];
  double red_nfa[kThreads / 64];
  int red_k[kThreads / 64];
};

// where the per-match arrays of one view live: LDS for up to kFMaxM putative matches ...
struct FShared {
  uint64_t key[kFMaxM];
  uint32_t idx[kFMaxM];
  int32_t vec_index[kFMaxM];
  int32_t best_inl[kFMaxM];
  float logc_n[kFMaxM + 1];
  float logc_k[kFMaxM + 1];
  FSmall small;
};
struct FStoreLds {
  FShared *S;
  __device__ __forceinline__ uint64_t *key() const { return S->key; }
  __device__ __forceinline__ uint32_t *idx() const { return S->idx; }
  __device__ __forceinline__ int32_t *vec_index() const { return S->vec_index; }
  __device__ __forceinline__ int32_t *best_inl() const { return S->best_inl; }
  __device__ __forceinline__ float *logc_n() const { return S->logc_n; }
  __device__ __forceinline__ float *logc_k() const { return S->logc_k; }
};
// ... and one of a few global-memory slots for a view with more (k_fmatrix_large): the reference has no limit on the
// matches of a pair (MatchUtils.cpp:346-355), a near-duplicate of a map frame reaches several thousand
constexpr int kFLargeMaxM = 65536;  // matches per view the slots hold (the log10 table and 16-bit query indices end there)
constexpr int kFLargeSlots = 8;
struct FStoreGlobal {
  uint64_t *k;
  uint32_t *i;
  int32_t *vi, *bi;
  float *ln, *lk;
  __device__ __forceinline__ uint64_t *key() const { return k; }
  __device__ __forceinline__ uint32_t *idx() const { return i; }
  __device__ __forceinline__ int32_t *vec_index() const { return vi; }
  __device__ __forceinline__ int32_t *best_inl() const { return bi; }
  __device__ __forceinline__ float *logc_n() const { return ln; }
  __device__ __forceinline__ float *logc_k() const { return lk; }
};

// F-matrix AC-RANSAC of ONE view by the whole workgroup (block-wide sort); `st` says where the per-match arrays are,
// `max_m` how many matches they hold.  Returns false when the view has more matches than that.
template <typename Store>
__device__ bool fmatrix_filter_view(const FFilterArgs &A, uint32_t v, Store st, FSmall &S, int max_m) {
  const int tid = threadIdx.x;
  const int m = (int)A.put_count[v];
  const uint32_t off = A.view_off[v];
  constexpr int s = 7;
  if (m < A.min_putative || m <= s) {  // localization.cpp:408-415 ; ACRANSAC: nData <= sizeSample
    if (tid == 0) A.geo_count[v] = 0;
    return true;
  }
  if (m > max_m) return false;
  // NormalizePoints(x, w, h) for both images
  const int w1 = (int)A.view_wh[2 * v], h1 = (int)A.view_wh[2 * v + 1];
  const int w2 = (int)A.qw, h2 = (int)A.qh;
  const double s1 = 1.0 / sqrt((double)(w1 * h1)), s2 = 1.0 / sqrt((double)(w2 * h2));
  const double t1x = -0.5 * (double)w1 * s1, t1y = -0.5 * (double)h1 * s1;
  const double t2x = -0.5 * (double)w2 * s2, t2y = -0.5 * (double)h2 * s2;
  const double Dg = sqrt((double)w2 * (double)w2 + (double)h2 * (double)h2);
  const double Ar = (double)w2 * (double)h2;
  const double logalpha0 = det_log10(2.0 * Dg / Ar / s2);
  const double max_thr = (A.precision * A.precision) * s2 * s2;
  const double loge0 = det_log10(3.0 * (double)(m - s));
  const uint32_t stream = A.view_id[v];
  const int P = next_pow2(m);

  auto point = [&](int p, double &x, double &y, double &u, double &w) {
    const uint32_t i = A.match_i[off + p];
    const uint32_t j = A.match_key[off + p] & 0xFFFFu;
    const float2 a = A.map_kpt[off + i];
    const float2 b = A.q_kpt6[j];
    x = s1 * (double)a.x + t1x;
    y = s1 * (double)a.y + t1y;
    u = s2 * (double)b.x + t2x;
    w = s2 * (double)b.y + t2y;
  };
  auto solve = [&](const int32_t *smp, double *models) -> int {
    double x1[14], x2[14];
    for (int i = 0; i < 7; ++i) point(smp[i], x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]);
    return seven_point(x1, x2, models);
  };

  logcombi_tables_block(s, m, A.L10, reinterpret_cast<double *>(st.key()), st.logc_n(), st.logc_k());  // the key array is free until the first sort

  double min_nfa = pos_inf();
  int n_in = 0;
  long n_iter = A.n_iter;
  long n_reserve = n_iter / 10;
  n_iter -= n_reserve;
  bool identity = true;
  int n_index = m;
  long pre_base = -1;

  for (long iter = 0; iter < n_iter; ++iter) {
    const double *models;
    int nm;
    if (identity) {
      if (pre_base < 0 || iter >= pre_base + kFPre) {
        __syncthreads();
        pre_base = iter;
        if (tid < kFPre) {
          int32_t smp[7];
          double mm[27];
          ac_sample<7>(nullptr, m, A.seed, STAGE_FMATRIX, stream, (uint32_t)(pre_base + tid), smp);
          const int k = solve(smp, mm);
          S.pre_nm[tid] = k;
          for (int q = 0; q < 9 * k; ++q) S.pre_models[tid][q] = mm[q];
        }
        __syncthreads();
      }
      models = S.pre_models[iter - pre_base];
      nm = S.pre_nm[iter - pre_base];
    } else {
      __syncthreads();
      if (tid == 0) {
        int32_t smp[7];
        double mm[27];
        ac_sample<7>(st.vec_index(), n_index, A.seed, STAGE_FMATRIX, stream, (uint32_t)iter, smp);
        const int k = solve(smp, mm);
        S.cur_nm = k;
        for (int q = 0; q < 9 * k; ++q) S.cur_models[q] = mm[q];
      }
      __syncthreads();
      models = S.cur_models;
      nm = S.cur_nm;
    }
    bool better = false;
    for (int k = 0; k < nm; ++k) {
      double M[9];
      for (int q = 0; q < 9; ++q) M[q] = models[9 * k + q];
      __syncthreads();  // key/idx of the previous model are no longer read
      for (int p = tid; p < P; p += kThreads) {
        uint64_t kv = ~0ull;
        if (p < m) {
          double x, y, u, w;
          point(p, x, y, u, w);
          kv = d2u(err_fmatrix(M, x, y, u, w));
        }
        st.key()[p] = kv;
        st.idx()[p] = (uint32_t)p;
      }
      __syncthreads();
      bitonic_sort(st.key(), st.idx(), P);
      const NfaBest b = best_nfa_block(st.key(), m, s, max_thr, logalpha0, 0.5, loge0, st.logc_n(), st.logc_k(), S.red_nfa,
                                       S.red_k);
      if (b.nfa < min_nfa) {
        better = true;
        min_nfa = b.nfa;
        n_in = b.k;
        for (int p = tid; p < n_in; p += kThreads) st.best_inl()[p] = (int32_t)st.idx()[p];
        if (tid < 9) S.best_model[tid] = M[tid];
      }
    }
    if ((better && min_nfa < 0.0) || (iter + 1 == n_iter && n_reserve)) {
      if (n_in == 0) {
        n_iter++;
        n_reserve--;
      } else {
        __syncthreads();
        for (int p = tid; p < n_in; p += kThreads) st.vec_index()[p] = st.best_inl()[p];
        n_index = n_in;
        identity = false;
        if (n_reserve) {
          n_iter = iter + 1 + n_reserve;
          n_reserve = 0;
        }
      }
    }
  }
  __syncthreads();
  if (min_nfa >= 0.0) n_in = 0;
  if ((double)n_in > 7 * 2.5) {
    for (int p = tid; p < n_in; p += kThreads) A.geo_idx[off + p] = (uint32_t)st.best_inl()[p];
    if (tid == 0) A.geo_count[v] = (uint32_t)n_in;
    if (A.geo_model && tid == 0) {  // errorMax = the residual of the last inlier (the list ascends by residual)
      double x, y, u, w;
      point(st.best_inl()[n_in - 1], x, y, u, w);
      double *gm = A.geo_model + 10 * (size_t)v;
      for (int q = 0; q < 9; ++q) gm[q] = S.best_model[q];
      gm[9] = err_fmatrix(S.best_model, x, y, u, w);
    }
  } else if (tid == 0) {
    A.geo_count[v] = 0;
  }
  return true;
}

struct FmatrixFilterBody {
  static constexpr int kGangThreads = kThreads;
  static __device__ __forceinline__ void run(FFilterArgsPacked P) {
    const FFilterArgs A = ffilter_expand(P);
    extern __shared__ unsigned char smem_raw[];
    FShared &S = *reinterpret_cast<FShared *>(smem_raw);
    const uint32_t v = A.view_sel ? A.view_sel[blockIdx.x] : blockIdx.x;
    const int m = (int)A.put_count[v];
    if (m <= A.skip_le) return;
    if (!fmatrix_filter_view(A, v, FStoreLds{&S}, S.small, kFMaxM)) {
      // more matches than the LDS form holds: queue the view for k_fmatrix_large
      if (threadIdx.x == 0) {
        A.geo_count[v] = 0;
        if (A.large_list) {
          const uint32_t slot = atomicAdd(A.large_count, 1u);
          A.large_list[slot] = v;
        } else {
          atomicOr(A.status, 1);
        }
      }
    }
  }
};
__global__ __launch_bounds__(kThreads) void k_fmatrix_filter(FFilterArgsPacked P) {
  FmatrixFilterBody::run(P);
}

// The views k_fmatrix_filter queued (more than kFMaxM putative matches): kFLargeSlots persistent workgroups, each
// owning one global-memory slot, take them in turn.  Same algorithm, same arithmetic, same results; the sort runs
// through L2 instead of LDS, which costs milliseconds for such a view instead of failing the query.
struct FLargeArgs {
  uint64_t *key;
  uint32_t *idx;
  int32_t *vec_index, *best_inl;
  float *logc_n, *logc_k;
  int slot_m;  // matches one slot holds: a power of two >= the map's longest view, at most kFLargeMaxM
};
struct FmatrixLargeBody {
  static constexpr int kGangThreads = kThreads;
  static __device__ __forceinline__ void run(FFilterArgsPacked P, FLargeArgs W) {
    const FFilterArgs A = ffilter_expand(P);
    __shared__ FSmall S;
    const uint32_t n = *A.large_count;
    const size_t o = (size_t)blockIdx.x * W.slot_m;
    FStoreGlobal st{W.key + o, W.idx + o, W.vec_index + o, W.best_inl + o, W.logc_n + (size_t)blockIdx.x * (W.slot_m + 1),
                    W.logc_k + (size_t)blockIdx.x * (W.slot_m + 1)};
    for (uint32_t t = blockIdx.x; t < n; t += gridDim.x) {
      const uint32_t v = A.large_list[t];
      if (!fmatrix_filter_view(A, v, st, S, W.slot_m) && threadIdx.x == 0) {
        A.geo_count[v] = 0;
        atomicOr(A.status, 1);  // more than 65 536 matches in one view
      }
      __syncthreads();
    }
  }
};
__global__ __launch_bounds__(kThreads) void k_fmatrix_large(FFilterArgsPacked P, FLargeArgs W) {
  FmatrixLargeBody::run(P, W);
}

// ---------------------------------------------------------------------------------------------------
// K3, fast form (views with at most kF2MaxM putative matches -- in practice all of them): the same AC-RANSAC,
// restructured so that nothing waits on a single lane.
//   * the 7-point solver runs wave-wide (wave_seven_point), 8 hypotheses at a time, one per wave;
//   * while sampling is still uniform the iterations are independent, so a batch of them is solved and their
//     models are evaluated speculatively, one MODEL per wave (residuals -> per-wave bitonic sort -> bestNFA), eight
//     side by side; the sequential acceptance rule of ACRANSAC is then replayed over the results in iteration
//     order, and the winner's inlier list is taken from the wave that evaluated it, or, where that wave has
//     evaluated another model since (or was another workgroup's), rebuilt by evaluating that one model again;
//   * after the switch to inlier sampling each iteration depends on the previous one: wave 0 solves, waves 0..2
//     evaluate the (up to 3) models side by side.
// Results are bit-identical to k_fmatrix_filter (same samples, same arithmetic per value, same tie rules).
// ---------------------------------------------------------------------------------------------------
// (kF2MaxM = 512 putative matches per view, kF2Batch = 32 uniform iterations per batch, kK3WideViews: forms.h)

// (W = waves per view: 16 for a query alone on the GPU -- a view's latency --, 4 when the GPU is shared: a workgroup of 16
// waves at 124 VGPRs is a compute unit's whole register file, i.e. it starts only on a compute unit nothing else runs on
// and nothing else runs beside it; at 8 the Hamming scans of the other queries keep three of their waves per SIMD, at
// 4 all of them.  Measured at 20 queries in flight in round 3, when the popcount scan filled the chip: 16 / 8 / 4 waves
// 3 259 / 3 413 / 3 460 queries/s -- K3 costs the others 13 us per query instead of 36.  With the matrix-core scan, on four
// hardware queues, the order is the opposite: 4 / 8 / 16 waves 3 695 / 3 924 / 4 115 queries/s, and the wide form 4 114
// (profiles/k3k5_candidates.txt): the chip has room and a query's time is the length of its chain.  A shared GPU now takes
// the wide form, launch_fmatrix_filter; W serves the lists it does not take and gang sessions.)
// (M = putative matches per view the form holds: 512 -- at most 8 residuals per lane in the register sort, 124 VGPRs --
// or, round 3, 1 024 for the views of a query that nearly duplicates a map frame: 16 per lane, more registers, launched
// only while such queries come, forms.h; they took the block-wide LDS form before, 0.4 ms per frame)
template <int W, int MaxM = kF2MaxM>
struct F2SharedT {
  static constexpr int kF2MaxM = MaxM;
  uint32_t idx[W][kF2MaxM];  // sorted match indices of the model each wave evaluated last
  int idx_model[W];          // ... which model: its flattened index in the current batch, or -1 (none of this batch's)
  double pts[4][kF2MaxM];  // normalised x, y of the map keypoint, u, w of the query keypoint (one plane each: a
                           // wave reading element p of 64 consecutive matches hits 64 different banks)
  int32_t vec_index[kF2MaxM];
  int32_t best_inl[kF2MaxM];
  float logc_n[kF2MaxM + 1];
  float logc_k[kF2MaxM + 1];
  double pre_models[kF2Batch][27];
  int pre_nm[kF2Batch];
  double res_nfa[kF2Batch][3];
  int res_k[kF2Batch][3];
  double best_model[9];
  int iter_end[kF2Batch];  // flattened index one past the last model of each iteration of the batch
  uint8_t flat_b[kF2Batch * 3], flat_k[kF2Batch * 3];
  unsigned int wide_ticket;  // the wide form: this workgroup's arrival number
};

// How often a view's best model got its sorted inlier list from the segment of the wave that evaluated it [0] / from
// wave 0 evaluating the model again [1] (fmatrix_fast.body.inc take_inliers), since the last reset: the tests tell the
// reuse from a permanent fall-back by it (sfmloc_debug_k3_list_counts).  One relaxed add by one thread per fetched list.
__device__ unsigned long long g_k3_list_counts[2];
__device__ __forceinline__ void k3_count_list(bool copied) {
  __hip_atomic_fetch_add(&g_k3_list_counts[copied ? 0 : 1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending bitonic sort of one wave's own (key, idx) segment; no workgroup barrier involved
__device__ void bitonic_sort_wave(uint64_t *kw, uint32_t *iw, int P) {
  const int lane = threadIdx.x & 63;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (P >> 1); t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i + j;
        const bool up = (i & k) == 0;
        const uint64_t ka = kw[i], kb = kw[l];
        const uint32_t ia = iw[i], ib = iw[l];
        const bool a_gt_b = pair_less(kb, ib, ka, ia);
        if (a_gt_b == up) {
          kw[i] = kb;
          kw[l] = ka;
          iw[i] = ib;
          iw[l] = ia;
        }
      }
      wave_lds_sync();
    }
  }
}

template <int W, int MaxM = kF2MaxM, bool Wide = false>
struct FmatrixFastBody {
  static constexpr int kGangThreads = W * 64;
  static __device__ __forceinline__ void run(FFilterArgsPacked packed) {
    const FFilterArgs A = ffilter_expand(packed);
    constexpr int kF2Waves = W, kF2Threads = W * 64, kF2MaxM = MaxM;
    constexpr bool kF2Wide = Wide;
    using F2Shared = F2SharedT<W, MaxM>;
#include "fmatrix_fast.body.inc"
  }
};
template <int W, int MaxM = kF2MaxM, bool Wide = false>
__global__ __launch_bounds__(W * 64) void k_fmatrix_fast(FFilterArgsPacked packed) {
  const FFilterArgs A = ffilter_expand(packed);
  constexpr int kF2Waves = W, kF2Threads = W * 64, kF2MaxM = MaxM;
  constexpr bool kF2Wide = Wide;
  using F2Shared = F2SharedT<W, MaxM>;
#include "fmatrix_fast.body.inc"
}

// ---------------------------------------------------------------------------------------------------
// K5: P3P AC-RANSAC as rounds of (evaluate a batch of hypotheses | replay the sequential rule)
// ---------------------------------------------------------------------------------------------------
// (K5's start -- the state machine's initial state, the normalised points, the logcombi tables -- is p3p_init_block,
// ransac_device.h: k_match_set_finish of K4 runs it too)
struct P3pInitBody {
  static constexpr int kGangThreads = kThreads;
  static __device__ __forceinline__ void run(P3pArgs A) {
    __shared__ double s_terms[kP3pMaxN / 2 + 1];
    p3p_init_block(A, (int)*A.ms_n, kThreads, s_terms);
  }
};
__global__ __launch_bounds__(kThreads) void k_p3p_init(P3pArgs A) {
  P3pInitBody::run(A);
}

constexpr int kP3pWaveSeg = kP3pMaxN / 4;  // elements one wave sorts when the four models run side by side
// More than kP3pMaxN correspondences (the reference has no limit, localization.cpp:479-509; a near-duplicate of a map
// frame with thousands of landmarks gets there): the residual sort of a hypothesis runs in a global-memory segment
// instead of LDS, and a round evaluates only the first kP3pLargeBatch hypotheses (that many segments exist).  Both
// kernels derive the round's size and the inlier-list stride from the same device-side n.
__device__ __forceinline__ int p3p_round_batch(int n, int batch) {
  return (n > kP3pMaxN && batch > kP3pLargeBatch) ? kP3pLargeBatch : batch;
}
// How many hypotheses the next round evaluates when the GPU is shared.  A round's hypotheses all sample from the current
// index set and everything after the first one that improves the model is thrown away.  Once sampling has switched to
// the best model's inliers, an iteration improves on the running minimum about as often as a new record appears in a
// random sequence: t iterations after the switch the next improvement is within the next m with probability m/(t+m).
// Evaluating 3t (at least 64) instead of a full batch finds it three times out of four and otherwise just advances; the
// acceptance rule is replayed exactly for any partition into rounds, so only the cost changes: ~2x fewer hypotheses
// evaluated for ~1.3x the rounds (+8 % queries per second at 12 in flight in round 2, on the popcount scan; the policy's
// constants hardly matter, profiles/r02_p3p_adaptive_policy.txt).  A query alone on the GPU keeps full batches: rounds
// are what its latency is made of.  With the matrix-core scan (20 in flight, four hardware queues, K3 wide; queries/s,
// profiles/k3k5_candidates.txt): this rule with the hypotheses prepared ahead 4 043, full batches 4 277, full batches
// prepared ahead 3 646, this rule WITHOUT preparing ahead 4 451 -- the shared GPU's rule now (make_p3p_args); floor 32 /
// 128, slope 2 / 6 and 12 rounds queued instead of 9 all within 1 % of it.
__device__ __forceinline__ int p3p_next_batch_limit(const P3pArgs &A, int identity, long iter, long switch_iter, int n) {
  // (more than 512 correspondences: a model that passes the NFA filter costs a block-wide sort, and right after the
  // switch nearly every hypothesis passes -- its reference is the FIRST meaningful model -- while everything behind the
  // round's first improvement is thrown away: small rounds first, also for a query alone on the GPU)
  const bool costly = next_pow2(n) >= 1024;
  if ((!A.adaptive_batch && !costly) || identity) return 1 << 30;
  const long t = iter - switch_iter;
  const long m = (A.adapt_quarters * t) / 4;
  const long floor_ = costly && !A.adaptive_batch ? 16 : A.adapt_floor;
  return (int)(m < floor_ ? floor_ : (m > kP3pBatchMax ? kP3pBatchMax : m));
}
__device__ __forceinline__ size_t p3p_inl_stride(int n, int max_n) { return n > kP3pMaxN ? (size_t)max_n : (size_t)kP3pMaxN; }

// (the small members first, then idx, then key: the SMALL form of the round -- below -- allocates only kP3pSmallN entries
// per wave of idx and nothing of key)
struct P3pShared {
  double models[48];
  P3pPrep prep;  // Kneip's intermediates + the quartic's roots (lane 0), read by the four model lanes
  int nm;
  double red_nfa[kThreads / 64];
  int red_k[kThreads / 64];
  double red_err[kThreads / 64];
  uint32_t idx[kP3pMaxN];
  uint64_t key[kP3pMaxN];
};
// The SMALL form of a round (k_p3p_round_small): match sets of at most kP3pSmallN correspondences, whose models are
// sorted in at most kP3pSmallN / 64 registers per lane and never filtered.  k_p3p_round holds every form of the
// evaluation -- up to 16 (key, index, two table values) per lane for the register sort, the LDS and global sorts, the
// filter -- and the compiler gives it 248 VGPRs: ONE of its waves takes half a SIMD's register file, i.e. the place of
// four waves of the Hamming scan (68 VGPRs) that other queries in flight are running, for the 30-90 us a round lasts,
// and a round is 64-256 workgroups.  That, not K5's instructions (a tenth of the scan's) nor its LDS, is what K5 cost
// the other queries.  The small form is the same code with the large cases compiled out.  The host queues a query's
// rounds before it knows the set's size (forms.h: the map's last queries were all small); a small round
// that finds a larger set returns at once, state untouched -- as if it had not been launched --, and
// ctx_resection_wait queues that query's rounds again in the full form.  The partition into rounds and the form of a
// launch change nothing in the result.

// A round's results go from the workgroup that computed them to the one that replays the round, which may sit on
// another XCD (another L2): they are written through (agent-scope stores), so that delivering them needs no L2
// write-back -- only the stores' completion: every storing wave runs s_waitcnt vmcnt(0) after its last store and the
// workgroup's barrier then orders all of those waits in front of the one lane that adds to the counter
// (p3p_round.body.inc; the barrier alone does not wait on vmcnt).

// ---------------------------------------------------------------------------------------------------
// The NFA filter.  A model of this round can only matter to the replay if its NFA is below the best NFA the round
// started from (st.min_nfa = B: the running minimum only goes down), and finding a model's NFA means sorting its n
// residuals -- 4 us for 256 correspondences in a wave's registers, 100 us for 2 000 in LDS, per model.  Whether a model
// CAN beat B is decided without sorting: with e_(k) the k-th smallest residual,
//     NFA(k) = loge0 + (logalpha0 + log10(e_(k) + eps)) (k - s) + logc_n[k] + logc_k[k]  <  B
//         <=>  e_(k) + eps  <  T_k := 10 ^ ((B - loge0 - logc_n[k] - logc_k[k]) / (k - s) - logalpha0)
//         <=>  #{ i : e_i + eps < T_k }  >=  k,
// so a model beats B only if SOME k has at least k residuals below T_k.  With T'_k = max_{j <= k} T_j (monotone, >= T_k:
// a weaker, still necessary condition) every residual is binned by binary search in the table, the bins are counted and
// prefix-summed, and the model passes iff some bin's running count reaches the bin's lowest k.  A model that fails
// reports NFA = +inf (exactly what the replay does with any NFA >= its running minimum: nothing); a model that passes
// is evaluated exactly as before, so every result the replay acts on has the bits it always had.  The table is
// computed with a safety margin of 1e-7 in the exponent (the exact test's rounding is ~1e-12), i.e. the filter never
// rejects a model whose exactly computed NFA is below B.  For n > 1024 the bins are 2 or 4 values of k wide (threshold
// of the bin's upper end against the bin's lowest k: weaker again, still necessary), which keeps the table at 8 KB.
// ---------------------------------------------------------------------------------------------------
constexpr int kP3pFilterBins = 1024;
// (the filter runs for next_pow2(n) >= this, i.e. from 257 correspondences on: below that a model's register sort costs
// about what the filter does)
constexpr int kP3pFilterMinP = 512;
struct P3pFilterLds {  // lives in P3pShared::key (32 KB), which is idle until a model is sorted in LDS
  double T[kP3pFilterBins];            // T' at each bin's upper end
  uint32_t hist[4][kP3pFilterBins + 4];
  double wave_max[kThreads / 64];
  int pass[4];
};
static_assert(sizeof(P3pFilterLds) <= sizeof(uint64_t) * kP3pMaxN, "the filter's tables live in the sort's key array");

__device__ __forceinline__ int p3p_filter_shift(int n) { return n <= kP3pFilterBins ? 0 : (n <= 2 * kP3pFilterBins ? 1 : 2); }

// raw thresholds: the maximum of T_k over the k of each bin, bins owned by the calling threads (any subset of the
// workgroup: thread `t` of `nt` takes bins t, t + nt, ...)
__device__ __forceinline__ void p3p_filter_raw(P3pFilterLds &F, int n, int s, double B, double logalpha0, double loge0,
                                               const float *__restrict__ logc_n, const float *__restrict__ logc_k, int t,
                                               int nt) {
  const int sh = p3p_filter_shift(n), w = 1 << sh;
  const int nb = (n >> sh) + 1;
  for (int j = t; j < nb; j += nt) {
    double m = 0.0;
    for (int k = j << sh; k < (j << sh) + w; ++k)
      if (k > s && k <= n) {
        const double x = (B - loge0 - (double)logc_n[k] - (double)logc_k[k]) / (double)(k - s) - logalpha0 + 1e-7;
        const double T = x > 300.0 ? pos_inf() : exp10(x);
        m = T > m ? T : m;
      }
    F.T[j] = m;
  }
}

// T' = running maximum over the bins; every thread of the workgroup calls it (two barriers inside)
__device__ __forceinline__ void p3p_filter_scan(P3pFilterLds &F, int n) {
  const int sh = p3p_filter_shift(n);
  const int nb = (n >> sh) + 1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int per = (kP3pFilterBins + 4 + kThreads - 1) / kThreads;  // bins per thread, contiguous
  double v[per];
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = tid * per + i;
    const double x = j < nb ? F.T[j] : 0.0;
    run = x > run ? x : run;
    v[i] = run;
  }
  double inc = run;  // inclusive running maximum across the wave's lanes
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(inc, off, 64);
    if (lane >= off) inc = o > inc ? o : inc;
  }
  double before = __shfl_up(inc, 1, 64);
  if (lane == 0) before = 0.0;
  if (lane == 63) F.wave_max[wv] = inc;
  __syncthreads();
  for (int q = 0; q < wv; ++q) before = F.wave_max[q] > before ? F.wave_max[q] : before;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = tid * per + i;
    if (j < nb) F.T[j] = v[i] > before ? v[i] : before;
  }
  __syncthreads();
}

// one wave, one model: can it beat B?  (every lane returns the verdict)
__device__ __forceinline__ bool p3p_filter_model(P3pFilterLds &F, int wv, const double (&M)[12], int n, int s,
                                                 const double *__restrict__ pt3d, const double *__restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int sh = p3p_filter_shift(n);
  const int nb = (n >> sh) + 1;
  uint32_t *h = F.hist[wv];
  for (int j = lane; j < nb; j += 64) h[j] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int steps = 0;
  while ((1 << steps) < nb + 1) ++steps;
  // four elements of a lane at a time: their residuals (two f64 divisions each) and their searches (dependent LDS reads)
  // interleave
  constexpr int U = 4;
  for (int p0 = 0; p0 < n; p0 += 64 * U) {
    double r[U];
    int lo[U], hi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + 64 * u + lane;
      const int pc = p < n ? p : n - 1;
      const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
      r[u] = e + (double)FLT_EPSILON;
      lo[u] = 0;
      hi[u] = nb;
    }
    // first bin whose threshold exceeds r (nb: none); T is non-decreasing
    for (int it = 0; it < steps; ++it) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int mid = (lo[u] + hi[u]) >> 1;
        const bool below = mid < nb && r[u] < F.T[mid < nb ? mid : nb - 1];
        const bool open = lo[u] < hi[u];
        hi[u] = (open && below) ? mid : hi[u];
        lo[u] = (open && !below) ? mid + 1 : lo[u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (p0 + 64 * u + lane < n && lo[u] < nb) atomicAdd(&h[lo[u]], 1u);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // running counts: each lane a contiguous run of bins, then across the lanes
  constexpr int per = (kP3pFilterBins + 4 + 63) / 64;
  uint32_t c[per];
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = lane * per + i;
    sum += j < nb ? h[j] : 0u;
    c[i] = sum;
  }
  uint32_t inc = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  const uint32_t before = inc - sum;
  bool any = false;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = lane * per + i;
    const int k_lo = (j << sh) > s + 1 ? (j << sh) : s + 1;          // lowest k of the bin that NFA ranges over
    const int k_hi = (j << sh) + (1 << sh) - 1;
    if (j < nb && k_hi > s && k_lo <= n && before + c[i] >= (uint32_t)k_lo) any = true;
  }
  return __ballot(any) != 0ull;
}

// one model, the whole workgroup: can it beat B?  (p3p_filter_model with the four waves sharing the elements and ONE
// table of counts; every thread returns the verdict; two barriers inside)
__device__ __forceinline__ bool p3p_filter_model_block(P3pFilterLds &F, const double (&M)[12], int n, int s,
                                                       const double *__restrict__ pt3d, const double *__restrict__ xn) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int sh = p3p_filter_shift(n);
  const int nb = (n >> sh) + 1;
  uint32_t *h = F.hist[0];
  for (int j = tid; j < nb; j += kThreads) h[j] = 0u;
  __syncthreads();
  int steps = 0;
  while ((1 << steps) < nb + 1) ++steps;
  constexpr int U = 4;
  for (int p0 = 0; p0 < n; p0 += kThreads * U) {
    double r[U];
    int lo[U], hi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + kThreads * u + tid;
      const int pc = p < n ? p : n - 1;
      const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
      r[u] = e + (double)FLT_EPSILON;
      lo[u] = 0;
      hi[u] = nb;
    }
    for (int it = 0; it < steps; ++it) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int mid = (lo[u] + hi[u]) >> 1;
        const bool below = mid < nb && r[u] < F.T[mid < nb ? mid : nb - 1];
        const bool open = lo[u] < hi[u];
        hi[u] = (open && below) ? mid : hi[u];
        lo[u] = (open && !below) ? mid + 1 : lo[u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (p0 + kThreads * u + tid < n && lo[u] < nb) atomicAdd(&h[lo[u]], 1u);
  }
  __syncthreads();
  // every wave walks the same table of counts and reaches the same verdict
  constexpr int per = (kP3pFilterBins + 4 + 63) / 64;
  uint32_t c[per];
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = lane * per + i;
    sum += j < nb ? h[j] : 0u;
    c[i] = sum;
  }
  uint32_t inc = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  const uint32_t before = inc - sum;
  bool any = false;
#pragma unroll
  for (int i = 0; i < per; ++i) {
    const int j = lane * per + i;
    const int k_lo = (j << sh) > s + 1 ? (j << sh) : s + 1;
    const int k_hi = (j << sh) + (1 << sh) - 1;
    if (j < nb && k_hi > s && k_lo <= n && before + c[i] >= (uint32_t)k_lo) any = true;
  }
  return __ballot(any) != 0ull;
}

// one model evaluated by one wave in its registers: residuals of elements r * 64 + lane, register sort, NFA minimum;
// the sorted indices go to iw[] (LDS).  -> r (NFA, k) and the k-th smallest residual.
// first_hit: P3pState::first_hit -- the wave gives up between its steps once an EARLIER hypothesis of the round
// is known to change the index set (the replay will not look at this one); the value is read by every lane from the same
// address and taken from the first lane, so the wave decides as one.
__device__ __forceinline__ bool p3p_overtaken(const unsigned *first_hit, int b) {
  // (nothing is in front of the round's first hypothesis; with this uniform early-out k_p3p_round_small also keeps the
  // 624 bytes of scratch it had while first_hit could be null -- 672 without it)
  if (b == 0) return false;
  const unsigned v = __hip_atomic_load(first_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)v) < (unsigned)b;
}
template <int E, int S = 3>  // S: the kernel's sample size (3: P3P, 6: the six-point resection)
__device__ __forceinline__ void p3p_eval_regs(const double (&M)[12], NfaBest &r, double &r_err, const double *__restrict__ pt3d,
                                              const double *__restrict__ xn, const float *__restrict__ logc_n,
                                              const float *__restrict__ logc_k, uint32_t *iw, int lane, int n, double logalpha0,
                                              double loge0, int stamp_round, int b, const unsigned *first_hit) {
  uint64_t key[E];
  uint32_t idx[E];
  float cn[E], ck[E];
  if (p3p_overtaken(first_hit, b)) return;  // (r stays "no model")
  nfa_tables_fetch<E>(cn, ck, n, logc_n, logc_k);  // in flight during the residuals and the sort
  // the wave is alone on its SIMD: the E residuals of a lane are computed without branches (clamped index, then a
  // select) so that their dependent f64 chains -- two divisions each -- interleave
#pragma unroll
  for (int rr = 0; rr < E; ++rr) {
    const int p = (rr << 6) + lane;
    const int pc = p < n ? p : n - 1;
    const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
    key[rr] = p < n ? d2u(e) : ~0ull;
    idx[rr] = (uint32_t)p;
  }
  STAMP_P3P(stamp_round, b, 6);
  if (p3p_overtaken(first_hit, b)) return;
  wave_sort_fast<E>(key, idx, iw);
  STAMP_P3P(stamp_round, b, 7);
  if (p3p_overtaken(first_hit, b)) return;
#pragma unroll
  for (int rr = 0; rr < E; ++rr) iw[(rr << 6) + lane] = idx[rr];
  r = best_nfa_regs_ilp<E>(key, n, S, pos_inf(), logalpha0, 1.0, loge0, cn, ck);
  if (r.k != 0x7FFFFFFF) r_err = u2d(sorted_key_at<E>(key, r.k - 1));
}

// entries of a sorted run of L keys (L a power of two) that come before x: those < x, or (le) those <= x
template <int L>
__device__ __forceinline__ int run_count_before(const uint64_t *run, uint64_t x, bool le) {
  int lo = 0, hi = L;
  constexpr int kSteps = (L == 64 ? 7 : L == 128 ? 8 : 9);  // L + 1 possible answers
  static_assert(L == 64 || L == 128 || L == 256, "run length");
#pragma unroll
  for (int it = 0; it < kSteps; ++it) {
    const int mid = (lo + hi) >> 1;
    const uint64_t v = run[mid < L ? mid : L - 1];
    const bool open = lo < hi;
    const bool before = le ? (v <= x) : (v < x);
    lo = (open && before) ? mid + 1 : lo;
    hi = (open && !before) ? mid : hi;
  }
  return lo;
}

// One model evaluated by the WHOLE workgroup (four waves; a "single" launch: one workgroup per model): wave j computes and
// sorts the residuals of elements 64 E j .. 64 E (j + 1) - 1 in its registers (wave_sort_fast, E <= 4 per lane), the four
// sorted runs are merged by rank through LDS -- an element's final position is its position in its own run plus, per
// other run, the number of that run's elements that come before it in the (key, index) order: runs of lower element
// indices win ties, which is the order of the one-wave sort -- and every thread takes its share of the NFA scan.  Up to
// 1 024 correspondences; the same residuals, order, candidates and first minimum as p3p_eval_regs, in a quarter of the
// dependent chain: one wave with 16 elements per lane sorts 1 024 residuals in ~16 us, four with 4 each in ~4 + ~2 for the
// merge.  `runs`: 256 E u64 of LDS, `fidx`: 256 E u32 (the sort's parking space, then the merged element indices).
// Every thread of the workgroup calls it (barriers inside) and gets the result.
template <int E>
__device__ __forceinline__ void p3p_eval_coop4(const double (&M)[12], NfaBest &res, double &res_err,
                                               const double *__restrict__ pt3d, const double *__restrict__ xn,
                                               const float *__restrict__ logc_n, const float *__restrict__ logc_k, int n,
                                               double logalpha0, double loge0, uint64_t *runs, uint32_t *fidx, double *red_nfa,
                                               int *red_k) {
  constexpr int L = 64 * E;
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int base = j * L;
  uint64_t key[E];
  uint32_t idx[E];
  float cn[E], ck[E];
#pragma unroll
  for (int rr = 0; rr < E; ++rr) {  // (the table entries of the merged positions this lane scans: in flight meanwhile)
    const int kk = base + (rr << 6) + lane + 1;
    cn[rr] = kk <= n ? logc_n[kk] : 0.0f;
    ck[rr] = kk <= n ? logc_k[kk] : 0.0f;
  }
#pragma unroll
  for (int rr = 0; rr < E; ++rr) {
    const int p = base + (rr << 6) + lane;
    const int pc = p < n ? p : n - 1;
    const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
    key[rr] = p < n ? d2u(e) : ~0ull;
    idx[rr] = 0u;
  }
  wave_sort_fast<E>(key, idx, fidx + base);
#pragma unroll
  for (int rr = 0; rr < E; ++rr) runs[base + (rr << 6) + lane] = key[rr];
  __syncthreads();
  int rank[E];
#pragma unroll
  for (int rr = 0; rr < E; ++rr) rank[rr] = (rr << 6) + lane;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u == j) continue;  // (uniform over the wave)
#pragma unroll
    for (int rr = 0; rr < E; ++rr) rank[rr] += run_count_before<L>(runs + u * L, key[rr], u < j);
  }
  __syncthreads();  // every rank is known: the runs may be overwritten
#pragma unroll
  for (int rr = 0; rr < E; ++rr) {
    runs[rank[rr]] = key[rr];
    fidx[rank[rr]] = (uint32_t)base + idx[rr];
  }
  __syncthreads();
  constexpr int s = 3;
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
  double l10[E];
  uint64_t mk[E];
#pragma unroll
  for (int rr = 0; rr < E; ++rr) mk[rr] = runs[base + (rr << 6) + lane];
#pragma unroll
  for (int rr = 0; rr < E; ++rr) l10[rr] = det_log10_inline(u2d(mk[rr]) + (double)FLT_EPSILON);
#pragma unroll
  for (int rr = 0; rr < E; ++rr) {
    const int kk = base + (rr << 6) + lane + 1;
    if (kk > s && kk <= n) {
      const double logalpha = logalpha0 + 1.0 * l10[rr];
      const double nfa = loge0 + logalpha * (double)(kk - s) + (double)cn[rr] + (double)ck[rr];
      if (nfa < lb) {
        lb = nfa;
        lk = kk;
      }
    }
  }
  const NfaBest wr = wave_reduce_nfa(lb, lk);
  if (lane == 0) {
    red_nfa[j] = wr.nfa;
    red_k[j] = wr.k;
  }
  __syncthreads();
  NfaBest r{red_nfa[0], red_k[0]};
#pragma unroll
  for (int u = 1; u < 4; ++u)
    if (red_nfa[u] < r.nfa || (red_nfa[u] == r.nfa && red_k[u] < r.k)) {
      r.nfa = red_nfa[u];
      r.k = red_k[u];
    }
  res = r;
  res_err = r.k != 0x7FFFFFFF ? u2d(runs[r.k - 1]) : pos_inf();
}

// The same for 1 025 .. 4 096 correspondences: NR = P / 1 024 runs of 256 per wave, sorted one after the other in the wave's
// registers and parked in LDS; then every element's rank among the 4 NR runs by binary search (a run of lower element
// indices wins ties), the scatter into the merged order, and the NFA scan, P / 256 positions per thread.  Replaces the
// block-wide bitonic sort in LDS for one-workgroup-per-model launches: 66 (78) barrier-separated stages over 2 048
// (4 096) elements, 110 us (250 us) per model, against ~25 us (~45 us) this way.  runs: P u64 of LDS, fidx: P u32.
template <int NR>
__device__ __forceinline__ void p3p_eval_coop4_multi(const double (&M)[12], NfaBest &res, double &res_err,
                                                     const double *__restrict__ pt3d, const double *__restrict__ xn,
                                                     const float *__restrict__ logc_n, const float *__restrict__ logc_k, int n,
                                                     double logalpha0, double loge0, uint64_t *runs, uint32_t *fidx,
                                                     double *red_nfa, int *red_k) {
  constexpr int E = 4, L = 256, R = 4 * NR;
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  uint64_t key[NR][E];
  uint32_t gidx[NR][E];
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    const int base = (j * NR + q) * L;
    uint32_t idx[E];
#pragma unroll
    for (int rr = 0; rr < E; ++rr) {
      const int p = base + (rr << 6) + lane;
      const int pc = p < n ? p : n - 1;
      const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
      key[q][rr] = p < n ? d2u(e) : ~0ull;
      idx[rr] = 0u;
    }
    wave_sort_fast<E>(key[q], idx, fidx + base);
#pragma unroll
    for (int rr = 0; rr < E; ++rr) {
      runs[base + (rr << 6) + lane] = key[q][rr];
      gidx[q][rr] = (uint32_t)base + idx[rr];
    }
  }
  __syncthreads();
  int rank[NR][E];
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int rr = 0; rr < E; ++rr) rank[q][rr] = (rr << 6) + lane;
  for (int u = 0; u < R; ++u) {
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const int mine = j * NR + q;
      if (u == mine) continue;  // (uniform over the wave)
#pragma unroll
      for (int rr = 0; rr < E; ++rr) rank[q][rr] += run_count_before<L>(runs + u * L, key[q][rr], u < mine);
    }
  }
  __syncthreads();  // every rank is known: the runs may be overwritten
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int rr = 0; rr < E; ++rr) {
      runs[rank[q][rr]] = key[q][rr];
      fidx[rank[q][rr]] = gidx[q][rr];
    }
  __syncthreads();
  constexpr int s = 3;
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
  // merged positions tid, tid + 256, ...: k = position + 1 (any split of the candidates gives the same first minimum)
  for (int pos = threadIdx.x; pos < n; pos += kThreads) {
    const int kk = pos + 1;
    if (kk > s) {
      const double ek = u2d(runs[pos]);
      const double logalpha = logalpha0 + 1.0 * det_log10_inline(ek + (double)FLT_EPSILON);
      const double nfa = loge0 + logalpha * (double)(kk - s) + (double)logc_n[kk] + (double)logc_k[kk];
      if (nfa < lb || (nfa == lb && kk < lk)) {
        lb = nfa;
        lk = kk;
      }
    }
  }
  const NfaBest wr = wave_reduce_nfa(lb, lk);
  if (lane == 0) {
    red_nfa[j] = wr.nfa;
    red_k[j] = wr.k;
  }
  __syncthreads();
  NfaBest r{red_nfa[0], red_k[0]};
#pragma unroll
  for (int u = 1; u < 4; ++u)
    if (red_nfa[u] < r.nfa || (red_nfa[u] == r.nfa && red_k[u] < r.k)) {
      r.nfa = red_nfa[u];
      r.k = red_k[u];
    }
  res = r;
  res_err = r.k != 0x7FFFFFFF ? u2d(runs[r.k - 1]) : pos_inf();
}

// one hypothesis: sample, solve, evaluate the (up to 4) models, leave the best one's NFA / inliers / model in the
// round's result arrays.  Executed by one workgroup of k_p3p_round -- or, in a WIDE launch (four workgroups per
// hypothesis: model m of hypothesis b is workgroup m * batch + b) and from 513 correspondences on, by four, one model each: a model's residuals are
// two f64 divisions per correspondence and a lone wave issues one instruction every ~5 cycles, so with a wave per model
// 2 000 correspondences are 32 per lane (45 us for the filter alone, 105 us for a model that has to be sorted), and a
// hypothesis's models wait for each other; with a workgroup per model it is 8 per thread, four times as many waves on the
// compute unit, and the four models of a hypothesis side by side.  Results go to slot 4 b + m; the replay takes the
// best model of each hypothesis (the first on ties, as the sequential loop over a hypothesis's models does).
// While no model exists at all (n_in == 0) the sequential rule, arriving at the end of the main phase, moves one
// iteration from the reserve to the budget and goes on: the iterations up to n_iter + n_reserve are then all run from
// the same (identity) index set.  P3P nearly always has a model after its first iteration; the six-point kernel on a
// degenerate scene (every sample coplanar) never has one, and a round that stopped at n_iter would hand the reserve
// over one iteration per round.  Its rounds (kSolver 1) therefore evaluate up to the end of the reserve while n_in == 0;
// the replay consumes them by the same rule, so the result is the sequential one.
template <int kSolver>
__device__ __forceinline__ long p3p_eval_end(const P3pState &st) {
  return (long)st.n_iter + ((kSolver == 1 && st.n_in == 0) ? (long)st.n_reserve : 0l);
}
// kSolver 0: P3P (three points, up to four models).  1: the six-point resection of an uncalibrated query ("resect6"
// below: six points, one model, solved ahead of the round by k_resect6_prepare -- a hypothesis always finds its model
// in prep_models); everything behind the solver is the same text with the sample size and the model count changed.
template <int kForm, int kSolver = 0>  // kForm 0: the full form (k_p3p_round), 1: small (k_p3p_round_small)
__device__ __forceinline__ void p3p_eval_hypothesis(const P3pArgs &A, int batch, int wide, unsigned char *smem_raw, int b,
                                                    int mdl) {
  constexpr bool kSmall = kForm == 1;
  const P3pState &st = *A.state;
  const int n = st.n;
  if (b >= p3p_round_batch(n, batch) || b >= st.batch_limit) return;
  const long it = (long)st.iter + b;
  if (it >= p3p_eval_end<kSolver>(st)) return;
  P3pShared &S = *reinterpret_cast<P3pShared *>(smem_raw);
  const int tid = threadIdx.x;
  constexpr int s = kSolver == 1 ? 6 : 3;
  const int P = next_pow2(n);
  // An earlier hypothesis of this round is already known to change the index set: whatever this one finds, the replay
  // will not look at it (it stops at the FIRST such hypothesis, which is that one or an earlier one).  Nothing is
  // evaluated, the slot reports "no model".  Only workgroups that start late see this -- i.e. while the GPU is shared.
  // (ONE lane reads the word and the workgroup decides on that value: the waves' own reads could straddle an update and
  // part of the workgroup would leave in front of the barriers below)
  // (the decision is taken behind the barrier that follows the solver / the fetch of the prepared models, below)
  __shared__ unsigned s_first_hit;
  // one model per workgroup: a wide launch with enough correspondences (and the LDS forms: n <= kP3pMaxN)
  const bool single = kSolver == 0 && !kSmall && wide && n <= kP3pMaxN;
  // (a wide launch that is not in single mode runs workgroups 0 .. batch - 1 only -- p3p_round.body.inc -- and is a plain
  // round: slot b, so that the inlier lists of a set above kP3pMaxN, whose stride is max_n, stay inside the 64 lists
  // ctx_p3p_reserve sizes them for)
  const int slot = single ? 4 * b + mdl : b;
#ifdef SFMLOC_STAMPS
  const int stamp_round = st.rounds;
#endif
  STAMP_P3P(stamp_round, b, 0);
  const size_t inl_stride = p3p_inl_stride(n, A.max_n);
  // where the block-wide sort of this hypothesis runs
  uint64_t *const skey = n > kP3pMaxN ? A.ws_key + (size_t)b * A.max_n : S.key;
  uint32_t *const sidx = n > kP3pMaxN ? A.ws_idx + (size_t)b * A.max_n : S.idx;
  // (register path of the full form: up to 256 correspondences, 4 per lane.  The 8- and 16-per-lane instantiations it used
  // to hold for plain launches on 257 .. 1 024 correspondences made the kernel 248 VGPRs for every launch; such sets take
  // the small form, a wide launch -- p3p_eval_coop4 -- or, in a plain launch of this form, the block-wide sort)
  const bool fast = kSmall || P <= 256;
  constexpr int wave_seg = kSmall ? kP3pSmallN : kP3pWaveSeg;  // entries of S.idx a wave owns
  const double logalpha0 = det_log10(3.14159265358979323846);
  const double loge0 = det_log10((kSolver == 1 ? 1.0 : 4.0) * (double)(n - s));  // log10(MAX_MODELS (n - s))
  // the NFA filter (above): only once a model exists, only while its tables fit the idle part of the LDS
  const double nfa_to_beat = st.min_nfa;
  // (the small form has no LDS for the tables: its models are sorted, which gives the same result)
  const bool filter = !kSmall && nfa_to_beat < pos_inf() && n <= kP3pMaxN && P >= kP3pFilterMinP;
  P3pFilterLds &F = *reinterpret_cast<P3pFilterLds *>(S.key);
  // "Prepared ahead" (p3p_prepare_ahead, below): the models of this hypothesis may be there already
  const bool have = st.prep_iter == st.iter && b < st.prep_n;
  if (filter) {
    if (have) p3p_filter_raw(F, n, s, nfa_to_beat, logalpha0, loge0, A.logc_n, A.logc_k, tid, kThreads);
    else if (tid >= 64)  // (wave 0 is busy: its lane 0 solves the P3P below)
      p3p_filter_raw(F, n, s, nfa_to_beat, logalpha0, loge0, A.logc_n, A.logc_k, tid - 64, kThreads - 64);
  }
  if (have) {
    if (tid < 48) S.models[tid] = A.prep_models[48 * (size_t)b + tid];
    if (tid == 0) S.nm = A.prep_nm[b];
  } else if (kSolver == 1) {
    // (cannot happen: k_resect6_prepare covers exactly the hypotheses of the round that follows it.  Reported, not
    // papered over: the query ends with SFMLOC_EHIP)
    if (tid == 0) {
      atomicOr(&A.state->status, 8);
      S.nm = 0;
    }
  } else if (tid == 0) {
    int32_t smp[3];
    ac_sample<3>(st.identity ? nullptr : A.vec_index, st.n_index, A.seed, STAGE_P3P, A.stream, (uint32_t)it, smp);
    double x[6], X[9];
    for (int i = 0; i < 3; ++i) {
      x[2 * i] = A.xn[2 * smp[i]];
      x[2 * i + 1] = A.xn[2 * smp[i] + 1];
      X[3 * i] = A.pt3d[3 * smp[i]];
      X[3 * i + 1] = A.pt3d[3 * smp[i] + 1];
      X[3 * i + 2] = A.pt3d[3 * smp[i] + 2];
    }
    STAMP_P3P(stamp_round, b, 1);
    S.nm = p3p_kneip_prepare(x, X, S.prep);
  }
  if (tid == 0)
    s_first_hit = __hip_atomic_load(&A.state->first_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  STAMP_P3P(stamp_round, b, 2);
  if (s_first_hit < (unsigned)b) {  // (uniform: one lane's read, seen by all behind the barrier)
    if (tid == 0) store_through(A.hyp_nfa + slot, pos_inf());
    return;
  }
  const int nm = S.nm;
  if (single && mdl >= nm) {  // (uniform over the workgroup) no such root
    if (tid == 0) store_through(A.hyp_nfa + slot, pos_inf());
    return;
  }
  if (kSolver == 0 && !have && tid < nm) p3p_kneip_model(S.prep, tid, S.models + 12 * tid);  // the four roots' models side by side
  if (filter) p3p_filter_scan(F, n);  // (two barriers inside: the models are visible behind them too)
  else __syncthreads();
  STAMP_P3P(stamp_round, b, 3);
  if (!fast || single) {
    STAMP_P3P(stamp_round, b, 6);   // (the register path stamps 6 / 7 around its sort)
  }
  // which models have to be evaluated: bit k = model k (one model per workgroup: bit mdl only)
  int pass_mask = single ? (1 << mdl) : 0xF;
  if (filter) {
    if (single) {
      double M[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) M[q] = S.models[12 * mdl + q];
      pass_mask = p3p_filter_model_block(F, M, n, s, A.pt3d, A.xn) ? (1 << mdl) : 0;
      __syncthreads();  // F (in S.key) is dead from here on
    } else {
      const int wv = tid >> 6;
      bool pass_mine = false;
      if (wv < nm) {
        double M[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = S.models[12 * wv + q];
        pass_mine = p3p_filter_model(F, wv, M, n, s, A.pt3d, A.xn);
      }
      if ((tid & 63) == 0) F.pass[wv] = pass_mine ? 1 : 0;
      __syncthreads();
      pass_mask = 0;
      for (int k = 0; k < 4; ++k) pass_mask |= F.pass[k] << k;
      __syncthreads();  // F (in S.key) is dead from here on: the LDS sort may overwrite it
    }
  }
  if (!fast || single) {
    STAMP_P3P(stamp_round, b, 7);   // LDS path: 3 -> 6 = table scan, 6 -> 7 = the filter, 7 -> 4 = the models that passed
  }
  double best = pos_inf();
  int best_k = 0, best_m = -1;
  double best_err = pos_inf();
  if (single) {
    // one model per workgroup: the four waves share the model (p3p_eval_coop4 / _multi; every set the LDS forms hold)
    // (behind the filter once more: has an earlier hypothesis been found to change the index set meanwhile?)
    __syncthreads();
    if (tid == 0) s_first_hit = __hip_atomic_load(&A.state->first_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_first_hit < (unsigned)b) pass_mask = 0;
    if ((pass_mask >> mdl) & 1) {  // (uniform over the workgroup)
      double M[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) M[q] = S.models[12 * mdl + q];
      NfaBest r{pos_inf(), 0x7FFFFFFF};
      double r_err = pos_inf();
      const double *pt3d = A.pt3d, *xn = A.xn;
      const float *logc_n = A.logc_n, *logc_k = A.logc_k;
      if (P <= 256) p3p_eval_coop4<1>(M, r, r_err, pt3d, xn, logc_n, logc_k, n, logalpha0, loge0, S.key, S.idx, S.red_nfa, S.red_k);
      else if (P == 512) p3p_eval_coop4<2>(M, r, r_err, pt3d, xn, logc_n, logc_k, n, logalpha0, loge0, S.key, S.idx, S.red_nfa, S.red_k);
      else if (P == 1024) p3p_eval_coop4<4>(M, r, r_err, pt3d, xn, logc_n, logc_k, n, logalpha0, loge0, S.key, S.idx, S.red_nfa, S.red_k);
      else if (P == 2048) p3p_eval_coop4_multi<2>(M, r, r_err, pt3d, xn, logc_n, logc_k, n, logalpha0, loge0, S.key, S.idx, S.red_nfa, S.red_k);
      else p3p_eval_coop4_multi<4>(M, r, r_err, pt3d, xn, logc_n, logc_k, n, logalpha0, loge0, S.key, S.idx, S.red_nfa, S.red_k);
      if (r.nfa < best) {
        best = r.nfa;
        best_k = r.k;
        best_m = mdl;
        best_err = r_err;
        int32_t *dst = A.hyp_inl + (size_t)slot * inl_stride;
        for (int p = tid; p < best_k; p += kThreads) store_through(dst + p, (int32_t)S.idx[p]);
      }
    }
    STAMP_P3P(stamp_round, b, 4);
  } else if (fast) {
    // register path: a model is evaluated by ONE wave, residuals sorted in its registers; the (up to 4) models of the
    // hypothesis side by side, one wave each -- or (one model per workgroup) wave 0 takes the workgroup's model
    const int wv = tid >> 6, lane = tid & 63;
    // (never in single mode: a one-model-per-workgroup launch took the branch above)
    const int my_model = wv;
    const bool mine = wv < nm;
    uint32_t *iw = S.idx + (size_t)wv * wave_seg;
    NfaBest r{pos_inf(), 0x7FFFFFFF};
    double r_err = pos_inf();
    if (mine && ((pass_mask >> my_model) & 1)) {
      double M[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) M[q] = S.models[12 * my_model + q];
      // (the lambda must not capture the kernel-argument struct: that would put all of it on the stack)
      const double *pt3d = A.pt3d, *xn = A.xn;
      const float *logc_n = A.logc_n, *logc_k = A.logc_k;
      if constexpr (kSmall) {
        const unsigned *first_hit = &A.state->first_hit;
        // (inlined: 152 VGPRs for the whole kernel, against 212 with the evaluation as a called function)
#ifndef SFMLOC_STAMPS
        const int stamp_round = 0;
#endif
        switch (P >> 6) {
          case 1: p3p_eval_regs<1, s>(M, r, r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0, stamp_round, b, first_hit); break;
          case 2: p3p_eval_regs<2, s>(M, r, r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0, stamp_round, b, first_hit); break;
          case 4: p3p_eval_regs<4, s>(M, r, r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0, stamp_round, b, first_hit); break;
          default: p3p_eval_regs<8, s>(M, r, r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0, stamp_round, b, first_hit); break;
        }
      } else {
        // (a lambda the compiler keeps out of line -- the text of p3p_eval_regs once more: with a call to that function in
        // it the compiler inlines all five instantiations and the kernel needs 256 VGPRs and a SIMD to itself)
#ifdef SFMLOC_STAMPS
        auto run = [&M, &r, &r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0, stamp_round, b](auto e_tag) {
#else
        auto run = [&M, &r, &r_err, pt3d, xn, logc_n, logc_k, iw, lane, n, logalpha0, loge0](auto e_tag) {
#endif
          constexpr int E = decltype(e_tag)::value;
          uint64_t key[E];
          uint32_t idx[E];
          float cn[E], ck[E];
          nfa_tables_fetch<E>(cn, ck, n, logc_n, logc_k);  // in flight during the residuals and the sort
#pragma unroll
          for (int rr = 0; rr < E; ++rr) {
            const int p = (rr << 6) + lane;
            const int pc = p < n ? p : n - 1;
            const double e = err_resection(M, pt3d[3 * pc], pt3d[3 * pc + 1], pt3d[3 * pc + 2], xn[2 * pc], xn[2 * pc + 1]);
            key[rr] = p < n ? d2u(e) : ~0ull;
            idx[rr] = (uint32_t)p;
          }
          STAMP_P3P(stamp_round, b, 6);
          wave_sort_fast<E>(key, idx, iw);
          STAMP_P3P(stamp_round, b, 7);
#pragma unroll
          for (int rr = 0; rr < E; ++rr) iw[(rr << 6) + lane] = idx[rr];
          r = best_nfa_regs_ilp<E>(key, n, s, pos_inf(), logalpha0, 1.0, loge0, cn, ck);
          if (r.k != 0x7FFFFFFF) r_err = u2d(sorted_key_at<E>(key, r.k - 1));
        };
        switch (P >> 6) {
          case 1: run(std::integral_constant<int, 1>{}); break;
          case 2: run(std::integral_constant<int, 2>{}); break;
          default: run(std::integral_constant<int, 4>{}); break;
        }
      }
    }
    if (lane == 0) {
      S.red_nfa[wv] = r.nfa;
      S.red_k[wv] = r.k;
      S.red_err[wv] = r_err;
    }
    __syncthreads();
    STAMP_P3P(stamp_round, b, 4);
    for (int k = 0; k < nm; ++k)
      if (S.red_nfa[k] < best) {  // strict: the first model of the hypothesis wins ties, as the sequential loop does
        best = S.red_nfa[k];
        best_k = S.red_k[k];
        best_m = k;
      }
    if (best_m >= 0) {
      const int w_best = best_m;
      best_err = S.red_err[w_best];
      int32_t *dst = A.hyp_inl + (size_t)slot * inl_stride;
      const uint32_t *src = S.idx + (size_t)w_best * wave_seg;
      for (int p = tid; p < best_k; p += kThreads) store_through(dst + p, (int32_t)src[p]);
    }
  } else
  for (int k = 0; k < nm; ++k) {
    if (!((pass_mask >> k) & 1)) continue;  // (uniform over the workgroup)
    double M[12];
    for (int q = 0; q < 12; ++q) M[q] = S.models[12 * k + q];
    __syncthreads();
    for (int p = tid; p < P; p += kThreads) {
      uint64_t kv = ~0ull;
      if (p < n)
        kv = d2u(err_resection(M, A.pt3d[3 * p], A.pt3d[3 * p + 1], A.pt3d[3 * p + 2], A.xn[2 * p], A.xn[2 * p + 1]));
      skey[p] = kv;
      sidx[p] = (uint32_t)p;
    }
    __syncthreads();
    bitonic_sort(skey, sidx, P);
    const NfaBest r = best_nfa_block(skey, n, s, pos_inf(), logalpha0, 1.0, loge0, A.logc_n, A.logc_k, S.red_nfa,
                                     S.red_k);
    if (r.nfa < best) {  // strict: the first model of the hypothesis wins ties, as the sequential loop does
      best = r.nfa;
      best_k = r.k;
      best_m = k;
      best_err = u2d(skey[r.k - 1]);
      int32_t *dst = A.hyp_inl + (size_t)slot * inl_stride;
      for (int p = tid; p < best_k; p += kThreads) store_through(dst + p, (int32_t)sidx[p]);
    }
  }
  if (!fast) {
    STAMP_P3P(stamp_round, b, 4);
  }
  if (tid == 0) {
    // (min_nfa < 0 from the switch on, so every improvement changes the index set; before it only a meaningful model does)
    if (best < nfa_to_beat && best < 0.0) atomicMin(&A.state->first_hit, (unsigned)b);
    store_through(A.hyp_nfa + slot, best);
    store_through(A.hyp_k + slot, best_k);
    store_through(A.hyp_err + slot, best_err);
    if (best_m >= 0)
      for (int q = 0; q < 12; ++q) store_through(A.hyp_model + 12 * slot + q, S.models[12 * best_m + q]);
  }
  STAMP_P3P(stamp_round, b, 5);
}

// ---------------------------------------------------------------------------------------------------
// K6 (north-star extension A13; absent from the reference, which never calls RefinePose): non-linear refinement
// of [R|t] on the inliers, intrinsics fixed -- Levenberg-Marquardt on the squared reprojection error with a left
// rotation increment.  The normal equations [J r]^T [J r] (7x7: J^T J, J^T r, r^T r) are accumulated on the
// matrix cores: v_mfma_f64_16x16x4_f64 takes four rows of M = [J | r] (padded to 16 columns) per instruction,
// and because A[i][k] = M[4s+k][i] and B[k][j] = M[4s+k][j] sit in the same lane (i = j = lane & 15, k = lane >> 4)
// one f64 per lane feeds both operands.  Executed by the whole workgroup (barriers), arithmetic by wave 0.
// ---------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct RefineShared {
  double H[7][8];
  double delta[6];
};

// kGenK: the intrinsic is a general upper-triangular K with K(2,2) = 1 -- what KRt_From_P recovers for an uncalibrated
// query -- given as Kg = {fx, skew, cx, fy, cy}; f / ppx / ppy are then unused.  The calibrated form is the text it was.
template <bool kGenK = false>
__device__ void normal_equations_wave0(const double *pt2d, const double *pt3d, const int32_t *inl, int n, double f,
                                       double ppx, double ppy, const double *Rm, const double *tv,
                                       RefineShared &S, const double *Kg = nullptr) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int k = tid >> 4, col = tid & 15;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int rows = 2 * n;
    for (int s4 = 0; s4 < rows; s4 += 4) {
      const int row = s4 + k;
      double m = 0.0;
      if (row < rows && col < 7) {
        const int p = inl[row >> 1];
        const double X = pt3d[3 * p], Y = pt3d[3 * p + 1], Z = pt3d[3 * p + 2];
        const double rx = (Rm[0] * X + Rm[1] * Y) + Rm[2] * Z;  // R X
        const double ry = (Rm[3] * X + Rm[4] * Y) + Rm[5] * Z;
        const double rz = (Rm[6] * X + Rm[7] * Y) + Rm[8] * Z;
        const double xc = rx + tv[0], yc = ry + tv[1], zc = rz + tv[2];
        const double iz = 1.0 / zc;
        // d(u or v)/d(Xc)
        double g0, g1, g2, res;
        if (kGenK) {
          if ((row & 1) == 0) {  // u = (fx xc + skew yc) / zc + cx
            const double num = Kg[0] * xc + Kg[1] * yc;
            g0 = Kg[0] * iz;
            g1 = Kg[1] * iz;
            g2 = -num * iz * iz;
            res = (num * iz + Kg[2]) - pt2d[2 * p];
          } else {  // v = fy yc / zc + cy
            g0 = 0.0;
            g1 = Kg[3] * iz;
            g2 = -Kg[3] * yc * iz * iz;
            res = (Kg[3] * yc * iz + Kg[4]) - pt2d[2 * p + 1];
          }
        } else if ((row & 1) == 0) {
          g0 = f * iz;
          g1 = 0.0;
          g2 = -f * xc * iz * iz;
          res = (f * xc * iz + ppx) - pt2d[2 * p];
        } else {
          g0 = 0.0;
          g1 = f * iz;
          g2 = -f * yc * iz * iz;
          res = (f * yc * iz + ppy) - pt2d[2 * p + 1];
        }
        // d(Exp(w) R X)/dw = -[R X]_x  ->  g^T (-[RX]_x) = ( RX x g )
        switch (col) {
          case 0: m = ry * g2 - rz * g1; break;
          case 1: m = rz * g0 - rx * g2; break;
          case 2: m = rx * g1 - ry * g0; break;
          case 3: m = g0; break;
          case 4: m = g1; break;
          case 5: m = g2; break;
          default: m = res; break;
        }
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(m, m, acc, 0, 0, 0);
    }
    // D[row = (lane>>4) + 4*reg][col = lane&15]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int drow = k + 4 * r;
      if (drow < 7 && col < 7) S.H[drow][col] = acc[r];
    }
  }
  __syncthreads();
}

// Exp(w) * R by Rodrigues' formula
__device__ void rotate_left(const double *w, const double *Rm, double *out) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double th = sqrt(th2);
  double a, b;  // Exp(w) = I + a [w]x + b [w]x^2
  if (th < 1e-8) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
  } else {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  }
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double W2[9], E[9];
  matmul3(W, W, W2);
  for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * W[i] + b * W2[i];
  matmul3(E, Rm, out);
}

// returns the final cost; Rm/tv are updated in place (identically in every thread)
template <bool kGenK = false>
__device__ double refine_pose_block(const double *pt2d, const double *pt3d, const int32_t *inl, int n, double f,
                                    double ppx, double ppy, double *Rm, double *tv, int max_iter, int *iters_out,
                                    const double *Kg = nullptr) {
  __shared__ RefineShared S;
  normal_equations_wave0<kGenK>(pt2d, pt3d, inl, n, f, ppx, ppy, Rm, tv, S, Kg);
  double H[6][6], g[6], cost = S.H[6][6];
  for (int i = 0; i < 6; ++i) {
    g[i] = S.H[i][6];
    for (int j = 0; j < 6; ++j) H[i][j] = S.H[i][j];
  }
  double lambda = 1e-4;
  int it = 0;
  for (; it < max_iter; ++it) {
    // (H + lambda diag(H)) d = -g   -- every thread solves the same 6x6 system (Gaussian elimination, partial pivoting)
    double A[6][7];
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 6; ++j) A[i][j] = H[i][j];
      A[i][i] = H[i][i] * (1.0 + lambda);
      A[i][6] = -g[i];
    }
    bool singular = false;
    for (int c = 0; c < 6; ++c) {
      int piv = c;
      for (int r = c + 1; r < 6; ++r)
        if (dabs(A[r][c]) > dabs(A[piv][c])) piv = r;
      if (!(dabs(A[piv][c]) > 0.0)) {
        singular = true;
        break;
      }
      if (piv != c)
        for (int j = c; j < 7; ++j) {
          const double t = A[c][j];
          A[c][j] = A[piv][j];
          A[piv][j] = t;
        }
      for (int r = c + 1; r < 6; ++r) {
        const double fct = A[r][c] / A[c][c];
        for (int j = c; j < 7; ++j) A[r][j] = A[r][j] - fct * A[c][j];
      }
    }
    if (singular) break;
    double d[6];
    for (int i = 5; i >= 0; --i) {
      double acc = A[i][6];
      for (int j = i + 1; j < 6; ++j) acc = acc - A[i][j] * d[j];
      d[i] = acc / A[i][i];
    }
    double Rn[9], tn[3];
    rotate_left(d, Rm, Rn);
    tn[0] = tv[0] + d[3];
    tn[1] = tv[1] + d[4];
    tn[2] = tv[2] + d[5];
    __syncthreads();  // S.H of the previous pass has been read by every thread
    normal_equations_wave0<kGenK>(pt2d, pt3d, inl, n, f, ppx, ppy, Rn, tn, S, Kg);
    const double c_new = S.H[6][6];
    if (c_new < cost) {
      const double rel = (cost - c_new) / cost;
      for (int i = 0; i < 9; ++i) Rm[i] = Rn[i];
      for (int i = 0; i < 3; ++i) tv[i] = tn[i];
      cost = c_new;
      for (int i = 0; i < 6; ++i) {
        g[i] = S.H[i][6];
        for (int j = 0; j < 6; ++j) H[i][j] = S.H[i][j];
      }
      lambda = lambda * 0.1;
      if (lambda < 1e-12) lambda = 1e-12;
      if (rel < 1e-10) {
        ++it;
        break;
      }
    } else {
      lambda = lambda * 10.0;
      if (lambda > 1e10) break;
    }
  }
  __syncthreads();
  *iters_out = it;
  return cost;
}

// The sequential acceptance rule of ACRANSAC replayed over one round's results; executed by ONE workgroup, the last of
// the round to deliver its hypothesis (k_p3p_round), so a round is a single launch.
struct P3pReplayShared {
  double nfa[kP3pBatchMax];
  double err[kP3pBatchMax];
  int k[kP3pBatchMax];
  unsigned char m[kP3pBatchMax];  // wide launches: which of a hypothesis's four slots holds its best model
  int first[kThreads / 64];
};
// wide4: the launch has four result slots per hypothesis (4 b + m) and all four were written (one model per workgroup);
// a wide launch whose query turned out small wrote slot 4 b only, a plain launch slot b
template <int kSolver>
__device__ __forceinline__ void p3p_replay_impl(const P3pArgs &A, int batch, int wide4, int slot_mul, P3pReplayShared &RS);
template <int kSolver = 0>
__device__ __forceinline__ void p3p_replay(const P3pArgs &A, int batch, int single_mode, P3pReplayShared &RS) {
  // (four result slots per hypothesis only in single mode; any other launch, wide or not, wrote slot b)
  p3p_replay_impl<kSolver>(A, batch, single_mode, single_mode ? 4 : 1, RS);
}
template <int kSolver>
__device__ __forceinline__ void p3p_replay_impl(const P3pArgs &A, int batch, int wide, int slot_mul, P3pReplayShared &RS) {
  P3pState &st = *A.state;
  const int tid = threadIdx.x;
#ifdef SFMLOC_STAMPS
  const int stamp_round = st.rounds;
#endif
  STAMP_SEL(stamp_round, 0);
  batch = p3p_round_batch(st.n, batch);  // what the round evaluated
  if (batch > st.batch_limit) batch = st.batch_limit;
  const size_t inl_stride = p3p_inl_stride(st.n, A.max_n);
  // every thread replays the same scalar state machine; only the copies are cooperative
  long iter0 = st.iter, n_iter = st.n_iter, n_reserve = st.n_reserve;
  const long switch_iter0 = st.switch_iter;
  const long n_iter_evaluated = p3p_eval_end<kSolver>(st);  // the round ran hypotheses iter0 <= it < min(iter0+batch, this)
  double min_nfa = st.min_nfa, errmax = st.errmax;
  int n_in = st.n_in, n_index = st.n_index, identity = st.identity;
  const int identity0 = identity;  // still sampling uniformly when the round began
  int best_b = -1;  // hypothesis of this batch that currently holds the best model
  long processed = 0;
  bool index_changed = false;
  // the replay is a dependent chain over up to 512 hypotheses: read their results from LDS, not from L2
  double *const s_nfa = RS.nfa;
  double *const s_err = RS.err;
  int *const s_k = RS.k;
  for (int b = tid; b < batch && b < kP3pBatchMax; b += kThreads) {
    const bool live = iter0 + b < n_iter_evaluated;
    int slot = slot_mul * b;
    if (wide && live) {  // the hypothesis's best model: strictly smaller NFA, the first model on ties
      slot = 4 * b;
      double v = A.hyp_nfa[slot];
      for (int mm = 1; mm < 4; ++mm) {
        const double o = A.hyp_nfa[4 * b + mm];
        if (o < v) {
          v = o;
          slot = 4 * b + mm;
        }
      }
    }
    RS.m[b] = (unsigned char)(slot & 3);
    s_nfa[b] = live ? A.hyp_nfa[slot] : pos_inf();
    // (a slot that reports +inf wrote nothing else)
    s_err[b] = live && s_nfa[b] < pos_inf() ? A.hyp_err[slot] : 0.0;
    s_k[b] = live && s_nfa[b] < pos_inf() ? A.hyp_k[slot] : 0;
  }
  __syncthreads();
  // The sequential rule only acts at two kinds of hypotheses: one whose NFA improves on the running minimum, and the
  // one that ends the uniform phase.  Everything in between is skipped by a block-wide "first index below the
  // minimum" search instead of a dependent 512-step loop.
  int *const s_first = RS.first;
  auto first_below = [&](int from, int limit, double thr) -> int {
    int mine = 0x7FFFFFFF;
    for (int b = from + tid; b < limit; b += kThreads)
      if (s_nfa[b] < thr) {
        mine = b;
        break;
      }
    for (int off = 32; off > 0; off >>= 1) mine = min(mine, __shfl_xor(mine, off, 64));
    __syncthreads();  // s_first of the previous search is no longer read
    if ((tid & 63) == 0) s_first[tid >> 6] = mine;
    __syncthreads();
    int r = s_first[0];
    for (int w = 1; w < kThreads / 64; ++w) r = min(r, s_first[w]);
    return r;
  };
  int b = 0;
  for (;;) {
    // hypotheses b .. limit-1 were evaluated and are within the budget
    long lim = n_iter - iter0;
    if (lim > n_iter_evaluated - iter0) lim = n_iter_evaluated - iter0;
    if (lim > batch) lim = batch;
    const int limit = (int)lim;
    if (b >= limit) break;
    int e = first_below(b, limit, min_nfa);
    if (n_reserve) {  // "it + 1 == n_iter" with budget in reserve
      const long eb = n_iter - 1 - iter0;
      if (eb >= b && eb < limit && eb < e) e = (int)eb;
    }
    if (e >= limit) {
      processed = limit;
      break;
    }
    const long it = iter0 + e;
    const double nfa = s_nfa[e];
    bool better = false;
    if (nfa < min_nfa) {
      better = true;
      min_nfa = nfa;
      n_in = s_k[e];
      errmax = s_err[e];
      best_b = e;
    }
    processed = e + 1;
    b = e + 1;
    if ((better && min_nfa < 0.0) || (it + 1 == n_iter && n_reserve)) {
      if (n_in == 0) {
        n_iter++;
        n_reserve--;
      } else {
        index_changed = true;
        n_index = n_in;
        identity = 0;
        if (n_reserve) {
          n_iter = it + 1 + n_reserve;
          n_reserve = 0;
        }
        break;  // later hypotheses of this batch sampled from the old index set
      }
    }
  }
  STAMP_SEL(stamp_round, 1);
  const int best_slot = best_b < 0 ? 0 : (wide ? 4 * best_b + (int)RS.m[best_b] : slot_mul * best_b);
  if (best_b >= 0) {
    const int32_t *src = A.hyp_inl + (size_t)best_slot * inl_stride;
    for (int p = tid; p < n_in; p += kThreads) A.best_inl[p] = src[p];
    if (index_changed)
      for (int p = tid; p < n_in; p += kThreads) A.vec_index[p] = src[p];
  } else if (index_changed) {
    // the index set switches to the inliers of a model found in an EARLIER round (end of the main phase)
    for (int p = tid; p < n_in; p += kThreads) A.vec_index[p] = A.best_inl[p];
  }
  // (the index set is read again below -- "Prepared ahead" -- by other waves of this workgroup: the stores have left)
  if (A.prep_ahead) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const bool done = (iter0 + processed >= n_iter);
  const long iter_next = iter0 + processed;
  const long switch_iter = (index_changed && identity0) ? iter_next : switch_iter0;
  const int next_limit = p3p_next_batch_limit(A, identity, iter_next, switch_iter, st.n);
  // how many of the coming round's hypotheses are solved here (none: every workgroup solves its own)
  int n_prep = 0;
  if (A.prep_ahead && !done) {
    n_prep = next_limit < kP3pBatchMax ? next_limit : kP3pBatchMax;
    if (n_prep > kP3pLaterBatch) n_prep = kP3pLaterBatch;  // (full batches: the limit is "none", the launch's size is not)
    n_prep = p3p_round_batch(st.n, n_prep);
    if ((long)n_prep > n_iter - iter_next) n_prep = (int)(n_iter - iter_next);
  }
  if (tid == 0) {
    st.prep_iter = (int)iter_next;
    st.prep_n = n_prep;
    st.iter = (int)(iter0 + processed);
    st.n_iter = (int)n_iter;
    st.n_reserve = (int)n_reserve;
    st.min_nfa = min_nfa;
    st.errmax = errmax;
    st.n_in = n_in;
    st.n_index = n_index;
    st.identity = identity;
    st.rounds += 1;
    st.switch_iter = (int)switch_iter;
    st.batch_limit = next_limit;
    st.first_hit = ~0u;
    if (best_b >= 0)
      for (int q = 0; q < 12; ++q) st.model[q] = A.hyp_model[12 * best_slot + q];
    if (done) st.done = 1;
    st.arrive = 0u;  // the next round counts from zero
  }
  STAMP_SEL(stamp_round, 2);
  // Prepared ahead.  In a round every workgroup spends its first 8-11 us with ONE lane solving its hypothesis's P3P --
  // a chain of ~2 500 dependent f64 instructions -- while the other 255 lanes wait, and a lone lane costs its SIMD as
  // many issue cycles as a full wave.  With prep_ahead (gang sessions; make_p3p_args) the workgroup that has just replayed the round
  // solves the COMING round's hypotheses instead, one per lane (the same scalar code on the same inputs: the same bits):
  // it knows the state they sample from, its 256 lanes take as long as one did, and the coming round's workgroups find
  // their four models in memory (p3p_eval_hypothesis: `have`).  Whatever the coming launch does not cover by these
  // (a larger batch, a state that moved on) is solved by its workgroup as before.  A query alone on the GPU keeps the
  // old form: the four roots' models side by side are 5 us shorter than one lane doing them in turn.
  if (n_prep > 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the index set as this workgroup has just written it, not an L1 line
    for (int h = tid; h < n_prep; h += kThreads) {
      int32_t smp[3];
      ac_sample<3>(identity ? nullptr : A.vec_index, n_index, A.seed, STAGE_P3P, A.stream, (uint32_t)(iter_next + h), smp);
      double x[6], X[9];
      for (int i = 0; i < 3; ++i) {
        x[2 * i] = A.xn[2 * smp[i]];
        x[2 * i + 1] = A.xn[2 * smp[i] + 1];
        X[3 * i] = A.pt3d[3 * smp[i]];
        X[3 * i + 1] = A.pt3d[3 * smp[i] + 1];
        X[3 * i + 2] = A.pt3d[3 * smp[i] + 2];
      }
      P3pPrep prep;
      const int nm = p3p_kneip_prepare(x, X, prep);
      double *M = A.prep_models + 48 * (size_t)h;
      for (int r = 0; r < nm; ++r) {
        double Mr[12];
        p3p_kneip_model(prep, r, Mr);
        for (int q = 0; q < 12; ++q) M[12 * r + q] = Mr[q];
      }
      A.prep_nm[h] = nm;
    }
  }
}

// One round of P3P AC-RANSAC in one launch: every workgroup evaluates one hypothesis and delivers it (release fence +
// counter); the workgroup that arrives last -- it sees every result (acquire fence) -- replays the sequential rule and
// writes the state of the next round.  Nobody waits for anybody, so there is no co-residency requirement; workgroups
// without a hypothesis (past the batch or the budget) only count themselves in.  A launch on a finished state returns at
// once (st.done is written by the previous launch's last workgroup, i.e. before this launch starts).
struct P3pRoundBody {
  static constexpr int kGangThreads = kThreads;
  static constexpr int kGangMinWaves = 4;  // (128 VGPRs, as k_p3p_round)
  static __device__ __forceinline__ void run(P3pArgs A, int batch, int wide) {
    constexpr int kForm = 0, kSolver = 0;
#include "p3p_round.body.inc"
  }
};
__global__ __launch_bounds__(kThreads, 4) void k_p3p_round(P3pArgs A, int batch, int wide) {
  constexpr int kForm = 0, kSolver = 0;
#include "p3p_round.body.inc"
}
// the small form (above, at P3pShared): at most kP3pSmallN correspondences, a fraction of the registers
struct P3pRoundSmallBody {
  static constexpr int kGangThreads = kThreads;
  static constexpr int kGangMinWaves = 4;
  static __device__ __forceinline__ void run(P3pArgs A, int batch, int wide) {
    constexpr int kForm = 1, kSolver = 0;
#include "p3p_round.body.inc"
  }
};
// (min. 4 waves per SIMD = at most 128 VGPRs: Kneip's solver spills -- one lane's chain, once per workgroup -- and the
// round fits beside four workgroups of the lean shortlist scan, 4 x 96 VGPRs per SIMD, without evicting one)
__global__ __launch_bounds__(kThreads, 4) void k_p3p_round_small(P3pArgs A, int batch, int wide) {
  constexpr int kForm = 1, kSolver = 0;
#include "p3p_round.body.inc"
}

// ---------------------------------------------------------------------------------------------------
// resect6: the six-point DLT resection of an uncalibrated query (include/sfmloc.h "Uncalibrated queries";
// tests/resect6_np.py restates every operation and the GPU tests compare bits).  A hypothesis is six 2D-3D
// correspondences: the 12 x 12 design matrix D (two rows per point, the 3D points translated so that the first sampled
// one is the origin), G = D^T D, a cyclic Jacobi eigen-solve of G with a FIXED number of sweeps (geom_device.h's
// jacobi_fixed, written for N = 12), the eigenvector of the smallest eigenvalue as the 3 x 4 model.  Only + - * / sqrt.
//
// Four lanes per hypothesis, sixteen hypotheses per wave.  G and V (2 x 144 doubles per hypothesis) do not fit a lane's
// registers next to anything else (576 VGPRs); they live in LDS (D, dead once G is formed, shares V's space: 39 KB per
// wave), hypothesis-minor with a row pitch of 13 entries, and the lanes of a group are 16 apart (lane = 16 g + h): one
// half of the wave -- what a 64-bit LDS access serves at once -- then holds two values of g whose entries are an odd
// number of 16-double rows apart (13 in the column phase, 1 in the row phase), i.e. 32 distinct doubles, all banks, no
// conflict.  Lane g of a group owns the rows
// (and, in the row phase, the columns) k = g, g + 4, g + 8 of every rotation's update, so the dependent chain of a sweep is
// a third of one lane's.  Every lane of a group computes the rotation's c and s itself from the same three entries (the
// same bits); the phases of a rotation are separated by wave-level LDS fences (a wave's LDS operations execute in
// order: only the compiler has to be kept from moving them).  Which lane computes an entry never changes its value.
// ---------------------------------------------------------------------------------------------------
constexpr int kR6Sweeps = 10;
constexpr int kR6PerWave = 16;          // hypotheses per wave (four lanes each)
constexpr double kR6RankTol = 1e-12;    // no model when the second smallest eigenvalue <= this * the largest
constexpr int kR6Pitch = 13;            // entries per matrix row in LDS (12 used)
struct R6Lds {
  double G[12 * kR6Pitch * kR6PerWave];  // [row * kR6Pitch + col][hypothesis]
  double V[12 * kR6Pitch * kR6PerWave];  // first the design matrix D, then V
};
static_assert(sizeof(R6Lds) <= 64 * 1024, "resect6: one wave's matrices in static LDS");

// x: the six sampled image points (normalised), X: their 3D points; every lane of the group holds the same values.
// Returns the number of models (0 or 1) and the model in M -- in every lane of the group.  Executed by the whole wave
// (slots without a hypothesis run on zeros).
__device__ __forceinline__ int resect6_solve_wave(R6Lds &L, const double (&x)[12], const double (&X)[18], double (&M)[12]) {
  const int lane = threadIdx.x & 63, h = lane & 15, g = lane >> 4;
  auto at = [h](int i, int j) { return (i * kR6Pitch + j) * kR6PerWave + h; };
  double *const LD = L.V;  // the design matrix, until G is formed
  const double X0 = X[0], Y0 = X[1], Z0 = X[2];
#pragma unroll 1
  for (int r = g; r < 12; r += 4) {  // rows 2 i and 2 i + 1: point i
    const int i = r >> 1;
    const double Xi = X[3 * i] - X0, Yi = X[3 * i + 1] - Y0, Zi = X[3 * i + 2] - Z0;
    const double u = (r & 1) ? x[2 * i + 1] : x[2 * i];
    const int o = (r & 1) ? 4 : 0, z = (r & 1) ? 0 : 4;
    LD[at(r, o)] = Xi;
    LD[at(r, o + 1)] = Yi;
    LD[at(r, o + 2)] = Zi;
    LD[at(r, o + 3)] = 1.0;
    LD[at(r, z)] = 0.0;
    LD[at(r, z + 1)] = 0.0;
    LD[at(r, z + 2)] = 0.0;
    LD[at(r, z + 3)] = 0.0;
    LD[at(r, 8)] = -(u * Xi);
    LD[at(r, 9)] = -(u * Yi);
    LD[at(r, 10)] = -(u * Zi);
    LD[at(r, 11)] = -u;
  }
  wave_lds_sync();
#pragma unroll 1
  for (int i = g; i < 12; i += 4)
#pragma unroll 1
    for (int j = 0; j < 12; ++j) {
      double acc = LD[at(0, i)] * LD[at(0, j)];
      for (int r = 1; r < 12; ++r) acc = acc + LD[at(r, i)] * LD[at(r, j)];
      L.G[at(i, j)] = acc;
    }
  wave_lds_sync();  // D has been read by every lane: its space becomes V
#pragma unroll 1
  for (int i = g; i < 12; i += 4)
    for (int j = 0; j < 12; ++j) L.V[at(i, j)] = i == j ? 1.0 : 0.0;
  wave_lds_sync();
#pragma unroll 1
  for (int sw = 0; sw < kR6Sweeps; ++sw)
#pragma unroll 1
    for (int p = 0; p < 11; ++p)
#pragma unroll 1
      for (int q = p + 1; q < 12; ++q) {
        const double apq = L.G[at(p, q)];
        const bool skip = apq == 0.0;
        const double theta = (L.G[at(q, q)] - L.G[at(p, p)]) / (2.0 * apq);
        const double ath = theta < 0.0 ? -theta : theta;
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (ath + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        wave_lds_sync();  // every lane has read the three entries
        for (int k = g; k < 12; k += 4) {  // G J: columns p and q
          const double akp = L.G[at(k, p)], akq = L.G[at(k, q)];
          const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
          L.G[at(k, p)] = skip ? akp : np_;
          L.G[at(k, q)] = skip ? akq : nq_;
        }
        wave_lds_sync();
        for (int k = g; k < 12; k += 4) {  // J^T (G J): rows p and q
          const double apk = L.G[at(p, k)], aqk = L.G[at(q, k)];
          const double np_ = c * apk - s * aqk, nq_ = s * apk + c * aqk;
          L.G[at(p, k)] = skip ? apk : np_;
          L.G[at(q, k)] = skip ? aqk : nq_;
        }
        wave_lds_sync();
        if (g == 0 && !skip) {
          L.G[at(p, q)] = 0.0;
          L.G[at(q, p)] = 0.0;
        }
        for (int k = g; k < 12; k += 4) {  // (rows of V: a lane's own, no other lane reads them before the end)
          const double vkp = L.V[at(k, p)], vkq = L.V[at(k, q)];
          const double np_ = c * vkp - s * vkq, nq_ = s * vkp + c * vkq;
          L.V[at(k, p)] = skip ? vkp : np_;
          L.V[at(k, q)] = skip ? vkq : nq_;
        }
        wave_lds_sync();
      }
  // the smallest eigenvalue (the first on ties), the smallest of the others, the largest
  int imin = 0;
  double dmin = L.G[at(0, 0)], dmax_ = dmin;
  for (int i = 1; i < 12; ++i) {
    const double d = L.G[at(i, i)];
    if (d < dmin) {
      dmin = d;
      imin = i;
    }
    dmax_ = d > dmax_ ? d : dmax_;
  }
  double dsec = pos_inf();
  for (int i = 0; i < 12; ++i) {
    const double d = L.G[at(i, i)];
    if (i != imin && d < dsec) dsec = d;
  }
  double Pn[12];
  for (int k = 0; k < 12; ++k) Pn[k] = L.V[at(k, imin)];
  // back to the untranslated 3D frame: P = P' [I | -X0]
  for (int r = 0; r < 3; ++r)
    Pn[4 * r + 3] = Pn[4 * r + 3] - ((Pn[4 * r] * X0 + Pn[4 * r + 1] * Y0) + Pn[4 * r + 2] * Z0);
  int behind = 0;
  for (int i = 0; i < 6; ++i) {
    const double w = ((Pn[8] * X[3 * i] + Pn[9] * X[3 * i + 1]) + Pn[10] * X[3 * i + 2]) + Pn[11];
    behind += w < 0.0 ? 1 : 0;
  }
  bool ok = dsec > kR6RankTol * dmax_;  // (false for NaN)
  for (int k = 0; k < 12; ++k) {
    ok = ok && is_finite(Pn[k]);
    M[k] = behind > 3 ? -Pn[k] : Pn[k];
  }
  return ok ? 1 : 0;
}

// the models of the round that follows on the stream: hypotheses st.iter .. st.iter + (what that round evaluates) - 1,
// into prep_models / prep_nm, which p3p_eval_hypothesis reads ("Prepared ahead": the same hand-over)
__global__ __launch_bounds__(64) void k_resect6_prepare(P3pArgs A, int batch) {
  __shared__ R6Lds L;
  P3pState &st = *A.state;
  if (st.done) return;
  const int n = st.n;
  long lim = p3p_round_batch(n, batch);
  if (lim > st.batch_limit) lim = st.batch_limit;
  if (lim > p3p_eval_end<1>(st) - st.iter) lim = p3p_eval_end<1>(st) - st.iter;
  if (lim > kP3pBatchMax) lim = kP3pBatchMax;
  const int lane = threadIdx.x & 63;
  const int h = (int)blockIdx.x * kR6PerWave + (lane & 15);
  if ((long)blockIdx.x * kR6PerWave >= lim) return;  // (uniform: nothing for this wave)
  const bool valid = h < lim;
  double x[12], X[18], M[12];
  for (int i = 0; i < 12; ++i) x[i] = 0.0;
  for (int i = 0; i < 18; ++i) X[i] = 0.0;
  if (valid) {
    int32_t smp[6];
    ac_sample<6>(st.identity ? nullptr : A.vec_index, st.n_index, A.seed, STAGE_RESECT6, A.stream, (uint32_t)(st.iter + h), smp);
    for (int i = 0; i < 6; ++i) {
      x[2 * i] = A.xn[2 * smp[i]];
      x[2 * i + 1] = A.xn[2 * smp[i] + 1];
      X[3 * i] = A.pt3d[3 * smp[i]];
      X[3 * i + 1] = A.pt3d[3 * smp[i] + 1];
      X[3 * i + 2] = A.pt3d[3 * smp[i] + 2];
    }
  }
  const int nm = resect6_solve_wave(L, x, X, M);
  if (valid && (lane >> 4) == 0) {
    for (int q = 0; q < 12; ++q) A.prep_models[48 * (size_t)h + q] = M[q];
    A.prep_nm[h] = nm;
  }
  if (blockIdx.x == 0 && lane == 0) {  // (the other workgroups read neither word)
    st.prep_iter = st.iter;
    st.prep_n = (int)lim;
  }
}

// the rounds of an uncalibrated query: k_p3p_round / k_p3p_round_small with the six-point kernel's constants
__global__ __launch_bounds__(kThreads, 4) void k_resect6_round(P3pArgs A, int batch, int wide) {
  constexpr int kForm = 0, kSolver = 1;
#include "p3p_round.body.inc"
}
__global__ __launch_bounds__(kThreads, 4) void k_resect6_round_small(P3pArgs A, int batch, int wide) {
  constexpr int kForm = 1, kSolver = 1;
#include "p3p_round.body.inc"
}

// ACRANSAC's epilogue + SfM_Localizer::Localize + localization.cpp:511-547, once per query after the last round
// what the host reads after the stream has drained: the record's head (state -- "done?" --, pose, status, view counts)
// and, of a finished query, the inlier pairs.  Written by the kernel itself into the pinned host record: a copy launch
// per query (and per refill of rounds) less.
__device__ void p3p_publish(const P3pArgs &A) {
  if (!A.host) return;
  const uint32_t *src = reinterpret_cast<const uint32_t *>(A.record);
  uint32_t *dst = reinterpret_cast<uint32_t *>(A.host);
  constexpr int head = (int)(offsetof(HostResult, pair_qfeat) / sizeof(uint32_t));
  for (int i = threadIdx.x; i < head; i += kThreads) dst[i] = src[i];
  const P3pState &st = *A.state;
  if (st.done && A.max_n <= kP3pMaxN) {  // (a regrown workspace keeps its pair lists outside the record)
    const int k = A.result->ok ? A.result->n_inliers : 0;
    for (int i = threadIdx.x; i < k; i += kThreads) {
      A.host->pair_qfeat[i] = A.record->pair_qfeat[i];
      A.host->pair_landmark[i] = A.record->pair_landmark[i];
    }
  }
}

struct P3pFinishBody {
  static constexpr int kGangThreads = kThreads;
  static __device__ __forceinline__ void run(P3pArgs A) {
    P3pState &st = *A.state;
    if (!st.done || st.finished) {  // rounds still to come, or nothing to estimate (k_p3p_init's verdict): just report
      p3p_publish(A);
      return;
    }
    const int tid = threadIdx.x;
    const double min_nfa = st.min_nfa, errmax = st.errmax;
    const int n_in = st.n_in;
#ifdef SFMLOC_STAMPS
    const int stamp_round = st.rounds;
#endif

    __shared__ double Msh[12];
    if (tid < 12) Msh[tid] = st.model[tid];
    __syncthreads();
    int n_final = n_in;
    if (min_nfa >= 0.0) n_final = 0;
    const bool resection = (double)n_final > 2.5 * (A.uncal ? 6 : 3);  // 2.5 * MINIMUM_SAMPLES
    const bool ok = resection && n_final > A.min_inliers;
    Pose &R = *A.result;
    if (ok)
      for (int p = tid; p < n_final; p += kThreads) {
        const int32_t c = A.best_inl[p];
        A.pair_qfeat[p] = A.ms_qfeat[c];
        A.pair_landmark[p] = A.ms_landmark[c];
        A.inlier_idx[p] = c;
      }
    // every thread computes the (tiny) pose epilogue redundantly so that the refinement can use block barriers
    const double inv_f = 1.0 / A.focal;
    double Pm[12];
    for (int j = 0; j < 4; ++j) {  // P = K * [R|t]
      Pm[j] = A.focal * Msh[j] + A.ppx * Msh[8 + j];
      Pm[4 + j] = A.focal * Msh[4 + j] + A.ppy * Msh[8 + j];
      Pm[8 + j] = Msh[8 + j];
    }
    if (n_final == 0)
      for (int j = 0; j < 12; ++j) Pm[j] = 0.0;
    double Kq[9], Rq[9], tq[3], cq[3];
    double refine_cost = 0.0;
    int refine_iters = 0;
    if (ok) {
      krt_from_p(Pm, Kq, Rq, tq);
      if (A.refine_pose && A.uncal) {
        // an uncalibrated query: R and t refined on the raw pixels with the RECOVERED K held fixed; P = K [R|t] again
        __syncthreads();
        const double Kg[5] = {Kq[0], Kq[1], Kq[2], Kq[4], Kq[5]};
        refine_cost = refine_pose_block<true>(A.pt2d, A.pt3d, A.best_inl, n_final, 0.0, 0.0, 0.0, Rq, tq, 20, &refine_iters,
                                              Kg);
        for (int j = 0; j < 4; ++j) {
          const double c0 = j < 3 ? Rq[j] : tq[0], c1 = j < 3 ? Rq[3 + j] : tq[1], c2 = j < 3 ? Rq[6 + j] : tq[2];
          Pm[j] = (Kg[0] * c0 + Kg[1] * c1) + Kg[2] * c2;
          Pm[4 + j] = Kg[3] * c1 + Kg[4] * c2;
          Pm[8 + j] = c2;
        }
      } else if (A.refine_pose) {
        __syncthreads();  // inlier_idx written above by all threads
        refine_cost = refine_pose_block(A.pt2d, A.pt3d, A.best_inl, n_final, A.focal, A.ppx, A.ppy, Rq, tq, 20,
                                        &refine_iters);
        for (int r = 0; r < 3; ++r) {  // P = K [R|t] of the refined pose
          for (int j = 0; j < 3; ++j) {
            Pm[4 * r + j] = (r == 0) ? A.focal * Rq[j] + A.ppx * Rq[6 + j]
                          : (r == 1) ? A.focal * Rq[3 + j] + A.ppy * Rq[6 + j]
                                     : Rq[6 + j];
          }
          Pm[4 * r + 3] = (r == 0) ? A.focal * tq[0] + A.ppx * tq[2] : (r == 1) ? A.focal * tq[1] + A.ppy * tq[2] : tq[2];
        }
        Kq[0] = A.focal; Kq[1] = 0.0; Kq[2] = A.ppx; Kq[3] = 0.0; Kq[4] = A.focal; Kq[5] = A.ppy;
        Kq[6] = 0.0; Kq[7] = 0.0; Kq[8] = 1.0;
      }
      center_from_rt(Rq, tq, cq);
    }
    if (tid == 0) {
      R.ok = ok ? 1 : 0;
      R.n_inliers = n_final;
      R.n_matches_2d3d = st.n;
      R.iterations = st.iter;
      R.nfa = min_nfa;
      R.status = st.status;
      R.reserved = refine_iters;
      R.error_max = (n_final > 0) ? sqrt(errmax) / inv_f : errmax;
      for (int j = 0; j < 12; ++j) R.P[j] = Pm[j];
      if (ok) {
        for (int j = 0; j < 9; ++j) {
          R.K[j] = Kq[j];
          R.R[j] = Rq[j];
        }
        for (int j = 0; j < 3; ++j) {
          R.t[j] = tq[j];
          R.center[j] = cq[j];
        }
        if (A.refine_pose) R.stage_seconds[0] = refine_cost;  // overwritten by the host; kept for sfmloc_pose_read
      }
      st.finished = 1;
    }
    __syncthreads();  // the record is complete
    p3p_publish(A);
    STAMP_SEL(stamp_round, 3);
  }
};
__global__ __launch_bounds__(kThreads) void k_p3p_finish(P3pArgs A) {
  P3pFinishBody::run(A);
}

// L10[i] = log10(i) for the logcombi tables, computed once per map on the device
__global__ void k_fill_log10(double *L10, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) L10[i] = (i == 0) ? 0.0 : det_log10((double)i);
}

// parity probes for the f64 building blocks (sfmloc_debug_math)
__global__ void k_debug_math(int op, const double *in, int n, int in_stride, double *out, int out_stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *x = in + (size_t)i * in_stride;
  double *o = out + (size_t)i * out_stride;
  switch (op) {
    case 0: o[0] = det_log10(x[0]); break;
    case 1: o[0] = sqrt(x[0]); o[1] = x[0] / x[1]; break;
    case 2: {
      double r[3] = {0, 0, 0};
      o[0] = (double)solve_cubic(x[0], x[1], x[2], x[3], r);
      o[1] = r[0]; o[2] = r[1]; o[3] = r[2];
    } break;
    case 3: solve_quartic_real(x, o); break;
    case 4: {
      double F[27];
      for (int k = 0; k < 27; ++k) F[k] = 0.0;
      o[0] = (double)seven_point(x, x + 14, F);
      for (int k = 0; k < 27; ++k) o[1 + k] = F[k];
    } break;
    case 5: {
      double M[48];
      for (int k = 0; k < 48; ++k) M[k] = 0.0;
      o[0] = (double)p3p_kneip(x, x + 6, M);
      for (int k = 0; k < 48; ++k) o[1 + k] = M[k];
    } break;
    case 6: {
      double c[3];
      krt_from_p(x, o, o + 9, o + 18);
      center_from_rt(o + 9, o + 18, c);
      o[21] = c[0]; o[22] = c[1]; o[23] = c[2];
    } break;
    case 7: {
      int32_t smp[7];
      const uint64_t seed = (uint64_t)x[0] | ((uint64_t)x[1] << 32);
      ac_sample<7>(nullptr, (int)x[2], seed, (uint32_t)x[3], (uint32_t)x[4], (uint32_t)x[5], smp);
      for (int k = 0; k < 7; ++k) o[k] = (double)smp[k];
    } break;
    case 10: o[0] = (double)round6_dev((float)x[0]); break;  // the .feat round trip of a coordinate
    default: break;
  }
}

// op 8: wave_seven_point, one wave per row (same input/output layout as op 4)
__global__ __launch_bounds__(64) void k_debug_wave7(const double *in, int n, int in_stride, double *out, int out_stride) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const double *x = in + (size_t)i * in_stride;
  double *o = out + (size_t)i * out_stride;
  const int lane = threadIdx.x & 63;
  int r = lane / 9;
  if (r > 6) r = 6;
  double f = 0.0;
  const int nm = wave_seven_point(x[2 * r], x[2 * r + 1], x[14 + 2 * r], x[14 + 2 * r + 1], &f);
  if (lane == 0) o[0] = (double)nm;
  if (lane < 27) o[1 + lane] = (lane < 9 * nm) ? f : 0.0;
}

// op 9: wave_sort_fast, one wave per row of P + 1 doubles (P = 64, 128, ... 2048 keys, then n: elements >= n are
// padding); out[p] = index of the element at sorted position p, out[P + p] = its key as a double
template <int E>
__device__ void debug_sort_row(const double *x, double *o, int n, uint32_t *low) {
  const int lane = threadIdx.x & 63;
  uint64_t key[E];
  uint32_t idx[E];
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int p = (r << 6) + lane;
    key[r] = p < n ? d2u(x[p]) : ~0ull;
    idx[r] = (uint32_t)p;
  }
  wave_sort_fast<E>(key, idx, low);
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int p = (r << 6) + lane;
    o[p] = (double)idx[r];
    o[64 * E + p] = u2d(key[r]);
  }
}
__global__ __launch_bounds__(64) void k_debug_sort(const double *in, int n_rows, int in_stride, double *out, int out_stride) {
  __shared__ uint32_t low[2048];
  const int i = blockIdx.x;
  if (i >= n_rows) return;
  const double *x = in + (size_t)i * in_stride;
  double *o = out + (size_t)i * out_stride;
  const int P = in_stride - 1;
  const int n = (int)x[P];
  switch (P >> 6) {
    case 1: debug_sort_row<1>(x, o, n, low); break;
    case 2: debug_sort_row<2>(x, o, n, low); break;
    case 4: debug_sort_row<4>(x, o, n, low); break;
    case 8: debug_sort_row<8>(x, o, n, low); break;
    case 16: debug_sort_row<16>(x, o, n, low); break;
    case 32: debug_sort_row<32>(x, o, n, low); break;
    default: break;
  }
}

// op 11: resect6_solve_wave, four lanes per row; in: x[12] (six image points), X[18]; out: the model count, the model
__global__ __launch_bounds__(64) void k_debug_resect6(const double *in, int n, int in_stride, double *out, int out_stride) {
  __shared__ R6Lds L;
  const int lane = threadIdx.x & 63;
  const int i = (int)blockIdx.x * kR6PerWave + (lane & 15);
  double x[12], X[18], M[12];
  for (int k = 0; k < 12; ++k) x[k] = 0.0;
  for (int k = 0; k < 18; ++k) X[k] = 0.0;
  if (i < n) {
    for (int k = 0; k < 12; ++k) x[k] = in[(size_t)i * in_stride + k];
    for (int k = 0; k < 18; ++k) X[k] = in[(size_t)i * in_stride + 12 + k];
  }
  const int nm = resect6_solve_wave(L, x, X, M);
  if (i < n && (lane >> 4) == 0) {
    double *o = out + (size_t)i * out_stride;
    o[0] = (double)nm;
    for (int k = 0; k < 12; ++k) o[1 + k] = M[k];
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int launch_fill_log10(double *d_L10, int n, hipStream_t s) {
  return dev_launch(k_fill_log10, dim3((n + 255) / 256), dim3(256), 0, s, d_L10, n);
}

int launch_debug_math(int op, const double *d_in, int n, int in_stride, double *d_out, int out_stride,
                      hipStream_t s) {
  if (op == 8)
    SFM_RC(dev_launch(k_debug_wave7, dim3(n), dim3(64), 0, s, d_in, n, in_stride, d_out, out_stride));
  else if (op == 9)
    SFM_RC(dev_launch(k_debug_sort, dim3(n), dim3(64), 0, s, d_in, n, in_stride, d_out, out_stride));
  else if (op == 11)
    SFM_RC(dev_launch(k_debug_resect6, dim3((n + kR6PerWave - 1) / kR6PerWave), dim3(64), 0, s, d_in, n, in_stride,
                      d_out, out_stride));
  else
    SFM_RC(dev_launch(k_debug_math, dim3((n + 63) / 64), dim3(64), 0, s, op, d_in, n, in_stride, d_out, out_stride));
  return SFMLOC_OK;
}

// global-memory slots of k_fmatrix_large, allocated the first time a map whose longest view exceeds the LDS form is used
static int ensure_fmatrix_large(Ctx *c) {
  if (c->fl_key) return SFMLOC_OK;
  Map *m = c->map;
  int slot_m = 64;
  while (slot_m < (int)m->max_view_rows && slot_m < kFLargeMaxM) slot_m <<= 1;
  c->fl_slot_m = slot_m;
  const size_t n = (size_t)kFLargeSlots * slot_m, n1 = (size_t)kFLargeSlots * (slot_m + 1);
  DevGroup g(&c->hbm_bytes);  // (all eight or none: fl_key stands for the set)
  g.add(c->fl_key, n);
  g.add(c->fl_idx, n);
  g.add(c->fl_vec_index, n);
  g.add(c->fl_best_inl, n);
  g.add(c->fl_logc_n, n1);
  g.add(c->fl_logc_k, n1);
  g.add(c->fl_count, 1);
  g.add(c->fl_list, (size_t)m->n_views + 1);
  if (!g.ok()) return g.rc();
  g.commit();
  return c->fl_count.zero(c->stream);  // (ahead of the launch that follows; later queries' reset kernel clears it)
}

// the argument list as the kernels take it (FFilterArgsPacked): the context's block on the device is rewritten when its
// content changes -- the first query, and the query after a lazily made buffer appeared -- and the host waits for that
// write (the block is read by launches queued behind it; a second change must not overtake them)
static_assert(sizeof(FFilterStatic) <= sizeof(Ctx::k3_static_host), "Ctx::k3_static_host holds an FFilterStatic");
static int k3_pack(Ctx *c, const FFilterArgs &A, FFilterArgsPacked *P) {
  FFilterStatic T;
  memset(&T, 0, sizeof(T));
  T.view_off = A.view_off;
  T.view_id = A.view_id;
  T.view_wh = A.view_wh;
  T.put_count = A.put_count;
  T.match_i = A.match_i;
  T.match_key = A.match_key;
  T.map_kpt = A.map_kpt;
  T.precision = A.precision;
  T.n_iter = A.n_iter;
  T.seed = A.seed;
  T.L10 = A.L10;
  T.geo_count = A.geo_count;
  T.geo_idx = A.geo_idx;
  T.geo_model = A.geo_model;
  T.large_count = A.large_count;
  T.large_list = A.large_list;
  T.status = A.status;
  // (a launch that does not merge leaves the block's merge pointers as they are: queries that alternate between the two
  // do not rewrite it)
  if (A.merge.enabled) T.merge = A.merge;
  else if (c->k3_static_valid) T.merge = reinterpret_cast<const FFilterStatic *>(c->k3_static_host)->merge;
  T.merge.enabled = 0;
  T.merge.view_sel = nullptr;
  T.merge.view_widx0 = nullptr;
  if (!c->d_k3_static) {
    int rc = c->d_k3_static.alloc(&c->hbm_bytes, sizeof(c->k3_static_host));
    if (rc) return rc;
  }
  if (!c->k3_static_valid || memcmp(&T, c->k3_static_host, sizeof(T)) != 0) {
    memcpy(c->k3_static_host, &T, sizeof(T));
    // (ahead of whatever a recording member has recorded -- nothing recorded reads the block before this call's launches
    // -- and without issuing it: a plain use of the stream would end the session's sharing for this member)
    hipStream_t s = c->stream.unordered();
    SFM_RC(c->d_k3_static.upload(c->k3_static_host, sizeof(T), s));
    SFM_HIP(hipStreamSynchronize(s));
    c->k3_static_valid = true;
  }
  P->st = reinterpret_cast<const FFilterStatic *>(c->d_k3_static.get());
  P->view_sel = A.view_sel;
  P->q_kpt6 = A.q_kpt6;
  P->merge_view_sel = A.merge.view_sel;
  P->merge_view_widx0 = A.merge.view_widx0;
  P->spec = A.spec;
  P->spec_arrive = A.spec_arrive;
  P->n_sel = A.n_sel;
  P->qw = A.qw;
  P->qh = A.qh;
  P->min_putative = A.min_putative;
  P->skip_le = A.skip_le;
  P->fast_min = A.fast_min;
  P->merge_enabled = A.merge.enabled;
  return SFMLOC_OK;
}

// one launch of k_fmatrix_fast<W, MaxM, kWide>: a workgroup per view, or (wide) per view and iteration of its first batch
template <int W, int MaxM, bool kWide>
static int launch_fmatrix_fast(Ctx *c, const FFilterArgs &A, int wide_b0) {
  using Sh = F2SharedT<W, MaxM>;
  static_assert(sizeof(Sh) <= 160 * 1024, "a workgroup's lists must fit a compute unit's LDS (160 KiB on gfx950)");
  FFilterArgsPacked P;
  SFM_RC(k3_pack(c, A, &P));
  return sfm_launch<FmatrixFastBody<W, MaxM, kWide>>(c, k_fmatrix_fast<W, MaxM, kWide>,
                                                     dim3(A.n_sel, (unsigned)wide_b0), dim3(W * 64),
                                                     (uint32_t)sizeof(Sh), P);
}

int launch_fmatrix_filter(Ctx *c, const Query *q, QueryPass &pass, uint32_t n_sel, bool all_views, int min_putative) {
  Map *m = c->map;
  if (n_sel == 0) return SFMLOC_OK;
  FFilterArgs A;
  A.view_sel = all_views ? nullptr : c->d_view_sel;
  A.n_sel = n_sel;
  A.view_off = m->d_view_off;
  A.view_id = m->d_view_id;
  A.view_wh = m->d_view_wh;
  A.put_count = c->d_view_count;
  A.match_i = c->d_match_i;
  A.match_key = c->d_match_key;
  A.map_kpt = m->d_kpt;
  A.q_kpt6 = q->d_kpt6;
  A.qw = q->width;
  A.qh = q->height;
  A.precision = m->params.geom_precision;
  A.n_iter = m->params.ransac_round;
  A.seed = m->params.seed;
  A.min_putative = min_putative >= 0 ? min_putative : m->params.min_putative;
  A.L10 = m->d_L10;
  A.geo_count = c->d_geo_count;
  A.geo_idx = c->d_geo_idx;
  A.geo_model = m->params.guided_matching ? c->d_geo_model : nullptr;
  A.status = c->d_status;
  c->geo_is_pairs = false;
  A.large_count = nullptr;
  A.large_list = nullptr;
  if (m->max_view_rows > (uint32_t)kFMaxM) {
    const bool fresh = c->fl_key == nullptr;
    int rc = ensure_fmatrix_large(c);
    if (rc) return rc;
    // (a memset on the context's stream would end a gang session's recording: every real map has views above 2 048 rows,
    // and with this line a session of image-in frames issued 93 launches, none of them shared -- the query's reset
    // kernel clears the counter; only the staged API, which has no reset kernel, clears it here)
    if (!pass.cleared && !fresh) SFM_RC(c->fl_count.zero(1, c->stream));
    A.large_count = c->fl_count;
    A.large_list = c->fl_list;
  }
  // which texts of k_fmatrix_fast run in front of k_fmatrix_filter, and on what (forms.h)
  K3In in;
  in.n_sel = n_sel;
  in.ransac_round = m->params.ransac_round;
  in.gang = c->stream.gang != nullptr;
  in.alone = c->k1_may_slice;
  in.merge_deferred = pass.merge_deferred;
  in.huge_credit = m->credits.k3_huge.load(std::memory_order_relaxed);
  in.big_credit = m->credits.k3_big.load(std::memory_order_relaxed);
  const K3Plan P = plan_k3(in, knobs());
  A.skip_le = P.skip_le;
  A.fast_min = -1;
  A.merge = MergeMaskedArgs{};
  A.spec = nullptr;
  A.spec_arrive = nullptr;
  pass.merge_deferred = false;
  if (P.k2 == K3Merge::kFolded) A.merge = pass.merge;
  if (P.k2 == K3Merge::kInFront) {
    int rc = launch_merge_masked_now(c, pass.merge, n_sel);
    if (rc) return rc;
  }
  if (P.wide) {
    if (!c->d_k3_spec) {
      DevGroup g(&c->hbm_bytes);
      g.add(c->d_k3_spec, (size_t)kK3WideViews * kF2Batch * sizeof(K3Spec));
      g.add(c->d_k3_arrive, (size_t)kK3WideViews);
      if (!g.ok()) return g.rc();
      g.commit();
      // (the last arrival clears its slot.  On the stream the launch below goes to, so that nothing waits for the device:
      // every context of a busy map gets here once.  Nothing a gang member has recorded touches the new buffer.)
      SFM_RC(c->d_k3_arrive.zero(kK3WideViews, c->stream.unordered()));
    }
    A.spec = reinterpret_cast<K3Spec *>(c->d_k3_spec.get());
    A.spec_arrive = c->d_k3_arrive;
    SFM_RC(P.max_m == kF2HugeM ? launch_fmatrix_fast<4, kF2HugeM, true>(c, A, P.wide_b0)
           : P.wide_waves == 8 ? launch_fmatrix_fast<8, kF2BigM, true>(c, A, P.wide_b0)
                               : launch_fmatrix_fast<4, kF2BigM, true>(c, A, P.wide_b0));
  } else {
    SFM_RC(P.waves == 16  ? launch_fmatrix_fast<16, kF2MaxM, false>(c, A, 1)
           : P.waves == 4 ? launch_fmatrix_fast<4, kF2MaxM, false>(c, A, 1)
                          : launch_fmatrix_fast<8, kF2MaxM, false>(c, A, 1));
    if (P.big) {
      FFilterArgs B = A;
      B.merge.enabled = 0;  // (the lists exist: the launch above built them)
      B.fast_min = kF2MaxM;
      SFM_RC(P.big_waves == 8 ? launch_fmatrix_fast<8, kF2BigM, false>(c, B, 1)
                              : launch_fmatrix_fast<4, kF2BigM, false>(c, B, 1));
    }
  }
  const size_t lds = sizeof(FShared);
  A.merge.enabled = 0;  // (the lists exist by now)
  FFilterArgsPacked PF;
  SFM_RC(k3_pack(c, A, &PF));
  SFM_RC(sfm_launch<FmatrixFilterBody>(c, k_fmatrix_filter, dim3(n_sel), dim3(kThreads), (uint32_t)lds, PF));
  if (A.large_list) {  // some view of this map can have more than kFMaxM matches: the queue's consumer
    FLargeArgs W;
    W.key = c->fl_key;
    W.idx = c->fl_idx;
    W.vec_index = c->fl_vec_index;
    W.best_inl = c->fl_best_inl;
    W.logc_n = c->fl_logc_n;
    W.logc_k = c->fl_logc_k;
    W.slot_m = c->fl_slot_m;
    SFM_RC(sfm_launch<FmatrixLargeBody>(c, k_fmatrix_large, dim3(kFLargeSlots), dim3(kThreads), 0, PF, W));
  }
  return SFMLOC_OK;
}


P3pArgs make_p3p_args(Ctx *c, const K5In &in) {
  Map *m = c->map;
  P3pArgs A;
  A.state = c->d_p3p_state;
  A.result = c->d_pose;
  A.record = reinterpret_cast<const HostResult *>(c->d_result.get());
  A.host = c->h_result;
  A.ms_n = c->d_ms_n;
  A.ms_qfeat = c->d_ms_qfeat;
  A.ms_landmark = c->d_ms_landmark;
  A.pt2d = c->d_pt2d;
  A.pt3d = c->d_pt3d;
  A.xn = c->d_xn;
  A.L10 = m->d_L10;
  A.logc_n = c->d_logc_n;
  A.logc_k = c->d_logc_k;
  A.vec_index = c->d_vec_index;
  A.best_inl = c->d_best_inl;
  A.hyp_nfa = c->d_hyp_nfa;
  A.hyp_k = c->d_hyp_k;
  A.hyp_err = c->d_hyp_err;
  A.hyp_model = c->d_hyp_model;
  A.prep_models = c->d_prep_models;
  A.prep_nm = c->d_prep_nm;
  A.hyp_inl = c->d_hyp_inl;
  A.pair_qfeat = c->d_pair_qfeat;
  A.pair_landmark = c->d_pair_landmark;
  A.inlier_idx = c->d_inlier_idx;
  // (a context that resects map views (adjust.hip) carries the view's own intrinsic; the query path uses the map's)
  A.focal = c->p3p_own_K ? c->p3p_K[0] : m->focal;
  A.ppx = c->p3p_own_K ? c->p3p_K[1] : m->ppx;
  A.ppy = c->p3p_own_K ? c->p3p_K[2] : m->ppy;
  // an uncalibrated query: no intrinsic at all.  The conditioning N1 of its image (sfmloc.h "Uncalibrated queries") has
  // the form of a K^-1 -- x / f - pp / f with f = sqrt(w h), pp = the image centre --, so the normalisation, the
  // un-normalisation of the model and of the error are the calibrated path's with these three numbers
  A.uncal = c->p3p_uncal ? 1 : 0;
  if (c->p3p_uncal) {
    A.focal = c->p3p_N[0];
    A.ppx = c->p3p_N[1];
    A.ppy = c->p3p_N[2];
  }
  A.max_iteration = m->params.p3p_max_iteration;
  A.min_resection_points = m->params.min_resection_points;
  A.min_inliers = m->params.min_inliers;
  A.max_n = (int)c->p3p_cap;
  A.ws_key = c->d_p3p_ws_key;
  A.ws_idx = c->d_p3p_ws_idx;
  A.ws_terms = c->d_p3p_terms;
  A.refine_pose = m->params.refine_pose;
  const K5QueryPlan Q = plan_k5_query(in, knobs());  // the shared-GPU round policy (forms.h)
  A.adaptive_batch = Q.adaptive_batch;
  A.prep_ahead = Q.prep_ahead;
  A.adapt_quarters = Q.adapt_quarters;
  A.adapt_floor = Q.adapt_floor;
  A.seed = m->params.seed;
  A.stream = c->p3p_stream;  // the AC-RANSAC sampling stream: 0 on the query path, the view id in adjust.hip
  return A;
}

int launch_p3p_init(Ctx *c) {
  if (c->p3p_init_fused) {  // k_match_set_finish has done it
    c->p3p_init_fused = false;
    return SFMLOC_OK;
  }
  P3pArgs A = make_p3p_args(c, k5_in(c));
  return sfm_launch<P3pInitBody>(c, k_p3p_init, dim3(1), dim3(kThreads), 0, A);
}

// Which launch form the P3P rounds went out in (sfmloc_debug_k5_round_counts): small, plain, wide.  Host side, one
// relaxed add per queued round; a six-point round is not counted.
static std::atomic<uint64_t> g_k5_round_counts[3];

int launch_p3p_round(Ctx *c, int batch) {
  const K5In in = k5_in(c);
  P3pArgs A = make_p3p_args(c, in);
  const size_t lds = sizeof(P3pShared);
  constexpr size_t lds_small = std::max(offsetof(P3pShared, idx) + 4 * kP3pSmallN * sizeof(uint32_t), sizeof(P3pReplayShared));
  static_assert(sizeof(P3pReplayShared) <= sizeof(P3pShared), "the replay reuses the round's LDS");
  const K5RoundPlan P = plan_k5_round(in, batch, knobs());
  if (P.six_point) {
    // an uncalibrated query (never in a gang session: capi.hip refuses): its round's models first, sixteen hypotheses
    // per wave, then the round
    hipStream_t s = (hipStream_t)c->stream;
    SFM_RC(dev_launch(k_resect6_prepare, dim3((P.batch + kR6PerWave - 1) / kR6PerWave), dim3(64), 0, s, A, P.batch));
    if (P.form == K5Form::kSmall)
      SFM_RC(dev_launch(k_resect6_round_small, dim3(P.grid), dim3(kThreads), (uint32_t)lds_small, s, A, P.batch, 0));
    else
      SFM_RC(dev_launch(k_resect6_round, dim3(P.grid), dim3(kThreads), (uint32_t)lds, s, A, P.batch, 0));
  } else if (P.form == K5Form::kSmall) {
    g_k5_round_counts[0].fetch_add(1, std::memory_order_relaxed);
    SFM_RC(sfm_launch<P3pRoundSmallBody>(c, k_p3p_round_small, dim3(P.grid), dim3(kThreads), (uint32_t)lds_small, A,
                                         P.batch, 0));
  } else {  // either launch shape gives the same bits
    g_k5_round_counts[P.form == K5Form::kWide ? 2 : 1].fetch_add(1, std::memory_order_relaxed);
    SFM_RC(sfm_launch<P3pRoundBody>(c, k_p3p_round, dim3(P.grid), dim3(kThreads), (uint32_t)lds, A, P.batch,
                                    P.form == K5Form::kWide ? 1 : 0));
  }
  return SFMLOC_OK;
}

int launch_p3p_finish(Ctx *c) {
  P3pArgs A = make_p3p_args(c, k5_in(c));
  return sfm_launch<P3pFinishBody>(c, k_p3p_finish, dim3(1), dim3(kThreads), 0, A);
}


int debug_k3_list_counts(int device, uint64_t *out, int reset) {
  SFM_HIP(hipSetDevice(device));
  SFM_HIP(hipDeviceSynchronize());
  unsigned long long v[2] = {0, 0};
  if (out) {
    SFM_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_k3_list_counts), sizeof(v)));
    out[0] = v[0];
    out[1] = v[1];
  }
  if (reset) {
    v[0] = v[1] = 0;
    SFM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_k3_list_counts), v, sizeof(v)));
  }
  return SFMLOC_OK;
}

int debug_k5_round_counts(int device, uint64_t *out, int reset) {
  SFM_HIP(hipSetDevice(device));
  SFM_HIP(hipDeviceSynchronize());
  for (int i = 0; i < 3; ++i) {
    const uint64_t v = reset ? g_k5_round_counts[i].exchange(0, std::memory_order_relaxed)
                             : g_k5_round_counts[i].load(std::memory_order_relaxed);
    if (out) out[i] = v;
  }
  return SFMLOC_OK;
}

#ifdef SFMLOC_STAMPS
int debug_stamps_read(int which, unsigned long long *out, size_t n) {
  hipDeviceSynchronize();
  hipError_t e = which == 0   ? hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_p3p), n * 8)
                 : which == 1 ? hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_sel), n * 8)
                              : hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_f), n * 8);
  return e == hipSuccess ? 0 : -1;
}
int debug_stamps_clear() {
  static unsigned long long z[16 * 256 * 8];
  hipDeviceSynchronize();
  hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_p3p), z, sizeof(z));
  hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_sel), z, 16 * 8 * 8);
  hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_f), z, 256 * 64 * 8);
  return 0;
}
#endif
}  // namespace sfmloc

extern "C" int sfmloc_debug_k3_list_counts(int device, uint64_t *out, int reset) {
  return sfmloc::debug_k3_list_counts(device, out, reset);
}
extern "C" int sfmloc_debug_k5_round_counts(int device, uint64_t *out, int reset) {
  return sfmloc::debug_k5_round_counts(device, out, reset);
}

#ifdef SFMLOC_STAMPS
extern "C" int sfmloc_debug_stamps_read(int which, unsigned long long *out, unsigned long long n) {
  return sfmloc::debug_stamps_read(which, out, (size_t)n);
}
extern "C" int sfmloc_debug_stamps_clear(void) { return sfmloc::debug_stamps_clear(); }
#endif
