// K4 of the query-localisation path for gfx950.
//
//   K4  k_emit_min / k_emit_win   matchProviderToMatchSet: per query feature keep the landmark whose match has the
//       k_match_set_finish        smallest descriptor distance, first one on ties   [SfMDataUtils.cpp:59-125]
#include "ransac_device.h"

namespace sfmloc {
namespace {

// ---------------------------------------------------------------------------------------------------
// K4: 2D-3D candidates and their de-duplication
// ---------------------------------------------------------------------------------------------------
// Every geometric match whose map feature has a landmark is a candidate for its query feature, ranked by
//   order key = dist << 48 | view_id << 24 | position in the view's geometric list
// (smaller is better; equal distance -> earlier in std::map iteration order = lower view id, then list order).
// dist = featDist[(v,q)][j] = d0 of the LAST putative match of the view that hit query feature j.
// matchProviderToMatchSet keeps ONE candidate per query feature (the minimum), so that is all a context -- or a shard --
// ever materialises: pass 1 (k_emit_min) computes every candidate's key and keeps the per-feature minimum with
// atomicMin, pass 2 (k_emit_win) turns the candidates that ARE the minimum into the part.  A part therefore holds at
// most one candidate per query feature (<= 65 535): no capacity can overflow however many geometric matches the views
// have, and a shard's exchange shrinks to its winners.
constexpr uint16_t kNoDist = 0xFFFFu;

struct EmitMinBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const uint32_t *view_sel, uint32_t n_sel, const uint32_t *view_off,
                                          const uint32_t *view_id, const uint32_t *put_count,
                                          const uint32_t *match_i, const uint32_t *match_key,
                                          const uint32_t *geo_count, const uint32_t *geo_idx,
                                          const uint32_t *geo_j /*null: geo_idx indexes the putative list; else
                                                                  (geo_idx, geo_j) = (map feature, query feature)
                                                                  of a guided match*/,
                                          const int32_t *row_landmark, unsigned long long *best64,
                                          uint16_t *geo_dist, uint32_t min_putative, uint32_t *view_stats) {
    // one workgroup (four waves) per selected view: the stage is a chain of dependent loads per candidate, so the waves
    // take 64 candidates each side by side instead of one wave walking them 64 at a time
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x;
    if (gw >= n_sel) return;
    const uint32_t v = view_sel ? view_sel[gw] : gw;
    const uint32_t ng = geo_count[v];
    if (threadIdx.x == 0) {  // the counts the reference prints (localization.cpp:416,458)
      if (put_count[v] >= min_putative) atomicAdd(&view_stats[0], 1u);
      if (ng > 0) atomicAdd(&view_stats[1], 1u);
      if (put_count[v] > (uint32_t)kF2MaxM) atomicMax(&view_stats[2], put_count[v]);  // (the host's hint for K3's launch forms)
    }
    if (ng == 0) return;
    const uint32_t off = view_off[v];
    const uint32_t np = put_count[v];
    // the view's putative keys in LDS (one segment per wave): the "last match with the same query feature" search
    // below is a dependent backward scan, far too slow against L2
    __shared__ uint32_t keys[kFMaxM];
    const bool staged = np <= (uint32_t)kFMaxM;
    if (staged) {
      for (uint32_t k = threadIdx.x; k < np; k += 256) keys[k] = match_key[off + k];
      __syncthreads();
    }
    // Round 3: from 128 putative matches on, "the last putative match with this query feature" is looked up in a hash
    // table (query feature -> largest list position, open addressing in LDS, at most half full) instead of walked to: the
    // walk is np / 2 dependent LDS reads per geometric match, and a frame that nearly duplicates a map view has 1 500 of
    // each -- 270 us per frame in the image-in leg, a few us now.  Same answer: the entry with the largest position.
    constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    __shared__ uint32_t tab[2 * kFMaxM];  // (query feature << 11) | position; positions < kFMaxM = 2 048
    static_assert(kFMaxM <= 2048, "a list position has 11 bits in the table's entries");
    const bool hashed = staged && np >= 128u;
    uint32_t tmask = 0;
    if (hashed) {
      uint32_t tsize = 256;
      while (tsize < 2u * np) tsize <<= 1;
      tmask = tsize - 1u;
      for (uint32_t e = threadIdx.x; e < tsize; e += 256) tab[e] = kEmpty;
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < np; k += 256) {
        const uint32_t jq = keys[k] & 0xFFFFu, val = (jq << 11) | k;
        uint32_t hsh = (jq * 2654435761u) >> 7 & tmask;
        for (;;) {
          uint32_t cur = __hip_atomic_load(&tab[hsh], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (cur == kEmpty) {
            cur = atomicCAS(&tab[hsh], kEmpty, val);
            if (cur == kEmpty) break;
          }
          if ((cur >> 11) == jq) {
            atomicMax(&tab[hsh], val);
            break;
          }
          hsh = (hsh + 1u) & tmask;
        }
      }
      __syncthreads();
    }
    const uint64_t vkey = (uint64_t)(view_id[v] & 0xFFFFFFu) << 24;
    for (uint32_t p0 = (threadIdx.x >> 6) * 64; p0 < ng; p0 += 256) {
      const uint32_t p = p0 + lane;
      if (p >= ng) continue;
      uint32_t i, j;
      if (geo_j) {
        i = geo_idx[off + p];
        j = geo_j[off + p];
      } else {
        const uint32_t pp = geo_idx[off + p];
        i = match_i[off + pp];
        j = match_key[off + pp] & 0xFFFFu;
      }
      uint16_t dist16 = kNoDist;
      if (row_landmark[off + i] >= 0 && hashed) {
        uint32_t hsh = (j * 2654435761u) >> 7 & tmask;
        for (;;) {
          const uint32_t cur = tab[hsh];
          if (cur == kEmpty) break;  // (no putative match of this view has this query feature: a guided match)
          if ((cur >> 11) == j) {
            dist16 = (uint16_t)(keys[cur & 2047u] >> 16);
            break;
          }
          hsh = (hsh + 1u) & tmask;
        }
      } else if (row_landmark[off + i] >= 0) {
        for (int32_t k = (int32_t)np - 1; k >= 0; --k) {  // last putative match with the same query feature
          const uint32_t kk = staged ? keys[k] : match_key[off + k];
          if ((kk & 0xFFFFu) == j) {
            dist16 = (uint16_t)(kk >> 16);
            break;
          }
        }
        // featDist has no entry for a query feature no putative match of this view hit (only possible for guided
        // matches): matchProviderToMatchSet then skips the match (SfMDataUtils.cpp:105-106) -> dist16 stays kNoDist
      }
      geo_dist[off + p] = dist16;
      if (dist16 != kNoDist)
        atomicMin(&best64[j], ((unsigned long long)dist16 << 48) | vkey | (unsigned long long)(p & 0xFFFFFFu));
    }
  }
};
__global__ __launch_bounds__(256) void k_emit_min(const uint32_t *view_sel, uint32_t n_sel, const uint32_t *view_off,
                                          const uint32_t *view_id, const uint32_t *put_count,
                                          const uint32_t *match_i, const uint32_t *match_key,
                                          const uint32_t *geo_count, const uint32_t *geo_idx,
                                          const uint32_t *geo_j /*null: geo_idx indexes the putative list; else
                                                                  (geo_idx, geo_j) = (map feature, query feature)
                                                                  of a guided match*/,
                                          const int32_t *row_landmark, unsigned long long *best64,
                                          uint16_t *geo_dist, uint32_t min_putative, uint32_t *view_stats) {
  EmitMinBody::run(view_sel, n_sel, view_off, view_id, put_count, match_i, match_key, geo_count, geo_idx, geo_j, row_landmark,
                   best64, geo_dist, min_putative, view_stats);
}

struct EmitWinBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const uint32_t *view_sel, uint32_t n_sel, const uint32_t *view_off,
                                          const uint32_t *view_id, const uint32_t *match_i,
                                          const uint32_t *match_key, const uint32_t *geo_count,
                                          const uint32_t *geo_idx, const uint32_t *geo_j,
                                          const int32_t *row_landmark, const uint32_t *landmark_id,
                                          const double *landmark_X, const unsigned long long *best64,
                                          const uint16_t *geo_dist, Candidate *cand, uint32_t cap,
                                          uint32_t *n_cand, int *status) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x;
    if (gw >= n_sel) return;
    const uint32_t v = view_sel ? view_sel[gw] : gw;
    const uint32_t ng = geo_count[v];
    if (ng == 0) return;
    const uint32_t off = view_off[v];
    const uint64_t vkey = (uint64_t)(view_id[v] & 0xFFFFFFu) << 24;
    for (uint32_t p0 = (threadIdx.x >> 6) * 64; p0 < ng; p0 += 256) {
      const uint32_t p = p0 + lane;
      bool has = false;
      uint32_t i = 0, j = 0;
      unsigned long long order = 0;
      if (p < ng) {
        const uint16_t d = geo_dist[off + p];
        if (d != kNoDist) {
          if (geo_j) {
            i = geo_idx[off + p];
            j = geo_j[off + p];
          } else {
            const uint32_t pp = geo_idx[off + p];
            i = match_i[off + pp];
            j = match_key[off + pp] & 0xFFFFu;
          }
          order = ((unsigned long long)d << 48) | vkey | (unsigned long long)(p & 0xFFFFFFu);
          has = best64[j] == order;
        }
      }
      // one atomic per wave step instead of one per winner
      const unsigned long long mask = __ballot(has);
      uint32_t slot0 = 0;
      if (lane == 0 && mask) slot0 = atomicAdd(n_cand, (uint32_t)__popcll(mask));
      slot0 = __shfl(slot0, 0, 64);
      if (!has) continue;
      const uint32_t slot = slot0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (slot >= cap) {  // cannot happen: at most one winner per query feature and cap >= SFMLOC_MAX_QUERY_ROWS
        atomicOr(status, 2);
        continue;
      }
      const int32_t lm = row_landmark[off + i];
      Candidate c;
      c.order = order;
      c.qfeat = j;
      c.landmark_id = landmark_id[lm];
      c.X[0] = landmark_X[3 * lm];
      c.X[1] = landmark_X[3 * lm + 1];
      c.X[2] = landmark_X[3 * lm + 2];
      cand[slot] = c;
    }
  }
};
__global__ __launch_bounds__(256) void k_emit_win(const uint32_t *view_sel, uint32_t n_sel, const uint32_t *view_off,
                                          const uint32_t *view_id, const uint32_t *match_i,
                                          const uint32_t *match_key, const uint32_t *geo_count,
                                          const uint32_t *geo_idx, const uint32_t *geo_j,
                                          const int32_t *row_landmark, const uint32_t *landmark_id,
                                          const double *landmark_X, const unsigned long long *best64,
                                          const uint16_t *geo_dist, Candidate *cand, uint32_t cap,
                                          uint32_t *n_cand, int *status) {
  EmitWinBody::run(view_sel, n_sel, view_off, view_id, match_i, match_key, geo_count, geo_idx, geo_j, row_landmark, landmark_id, landmark_X, best64, geo_dist, cand, cap, n_cand, status);
}

// A "part" is what one shard contributes for one query: 16-byte header {u32 n_cand, pad} + cap candidates.
// The selection kernels run over n_parts parts laid out back to back (n_parts = 1 on a single GPU; after the
// all-gather it is the number of shards).  Candidate c of part p has the global index p*cap + c.
//
// PACKED parts (the multi-GPU exchange, sfmloc_shard_export_packed): one buffer per shard for a whole batch of B
// queries -- header {u32 total, n_queries, budget, flags}, u32 count[B], u32 offset[B], then (16-byte aligned) the
// candidates of all B queries back to back in arrival order; query i's are [offset[i], offset[i] + count[i]).  The
// kernels address a candidate of part p as p*cap + c with cap = the budget and c counted from the start of the
// buffer's candidate area, so the two layouts differ only in where a part's range lies.
struct PartLayout {
  uint32_t packed_b;  // 0 = plain part; else B of the packed layout
  uint32_t qi;        // query index inside the packed batch
};
__host__ __device__ __forceinline__ uint64_t packed_cands_offset(uint32_t n_queries) {
  return (16ull + 8ull * n_queries + 15ull) & ~15ull;
}
__device__ __forceinline__ const Candidate *part_cands(const unsigned char *parts, uint64_t part_bytes, uint32_t p,
                                                       PartLayout L) {
  return reinterpret_cast<const Candidate *>(parts + (uint64_t)p * part_bytes +
                                             (L.packed_b ? packed_cands_offset(L.packed_b) : (uint64_t)kPartHeaderBytes));
}
// candidates [c0, c1) of part p belong to this query
__device__ __forceinline__ void part_range(const unsigned char *parts, uint64_t part_bytes, uint32_t p, uint32_t cap,
                                           PartLayout L, uint32_t *c0, uint32_t *c1) {
  const uint32_t *h = reinterpret_cast<const uint32_t *>(parts + (uint64_t)p * part_bytes);
  if (L.packed_b) {
    const uint32_t n = h[4 + L.qi], off = h[4 + L.packed_b + L.qi];
    *c0 = min(off, cap);
    *c1 = min(off + n, cap);
  } else {
    *c0 = 0;
    *c1 = min(h[0], cap);
  }
}

struct CandidatesMinBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const unsigned char *parts, uint32_t n_parts,
                                                uint64_t part_bytes, uint32_t cap, uint32_t nq,
                                                unsigned long long *best, int *status, PartLayout L) {
    for (uint32_t p = blockIdx.y; p < n_parts; p += gridDim.y) {
      const Candidate *cand = part_cands(parts, part_bytes, p, L);
      uint32_t c0, c1;
      part_range(parts, part_bytes, p, cap, L, &c0, &c1);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t *h = reinterpret_cast<const uint32_t *>(parts + (uint64_t)p * part_bytes);
        // a shard produced more candidates than its part holds (packed: than the batch's budget, or than a context holds)
        if (L.packed_b ? (h[0] > cap || h[3] != 0) : (h[0] > cap)) atomicOr(status, 2);
      }
      for (uint32_t c = c0 + blockIdx.x * blockDim.x + threadIdx.x; c < c1; c += gridDim.x * blockDim.x)
        if (cand[c].qfeat < nq) atomicMin(&best[cand[c].qfeat], (unsigned long long)cand[c].order);
    }
  }
};
__global__ __launch_bounds__(256) void k_candidates_min(const unsigned char *parts, uint32_t n_parts,
                                                uint64_t part_bytes, uint32_t cap, uint32_t nq,
                                                unsigned long long *best, int *status, PartLayout L) {
  CandidatesMinBody::run(parts, n_parts, part_bytes, cap, nq, best, status, L);
}

struct MatchSetFinishBody {
  static constexpr int kGangThreads = 1024;
  static __device__ __forceinline__ void run(const unsigned char *parts, uint32_t n_parts,
                                                  uint64_t part_bytes,
                                                  uint32_t cap, const unsigned long long *best,
                                                  uint32_t *winner, uint32_t nq, const float2 *q_kpt,
                                                  uint32_t *ms_n, uint32_t *ms_qfeat, uint32_t *ms_landmark,
                                                  double *pt2d, double *pt3d, int radial_k3, double f, double ppx,
                                                  double ppy, double k1, double k2, double k3, PartLayout L,
                                                  P3pArgs init /*K5's start, by this workgroup: one launch less*/) {
    // one workgroup; winners are compacted in query-feature order, 1024 features per pass (a pass is a chain of
    // dependent loads, so fewer, wider passes)
    __shared__ uint32_t wave_cnt[16];
    __shared__ uint32_t base_s;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    // which candidate holds each query feature's minimum (the parts hold winners only -- a few
    // hundred candidates each --, so the one workgroup that compacts them can also find them: one launch less)
    for (uint32_t p = 0; p < n_parts; ++p) {
      const Candidate *cand = part_cands(parts, part_bytes, p, L);
      uint32_t c0, c1;
      part_range(parts, part_bytes, p, cap, L, &c0, &c1);
      for (uint32_t c = c0 + threadIdx.x; c < c1; c += 1024)
        if (cand[c].qfeat < nq && best[cand[c].qfeat] == (unsigned long long)cand[c].order)
          winner[cand[c].qfeat] = p * cap + c;
    }
    __syncthreads();
    for (uint32_t j0 = 0; j0 < nq; j0 += 1024) {
      const uint32_t j = j0 + threadIdx.x;
      const bool has = j < nq && best[j] != ~0ull;
      const unsigned long long mask = __ballot(has);
      if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
      __syncthreads();
      uint32_t pre = base_s;
      for (uint32_t w = 0; w < wave; ++w) pre += wave_cnt[w];
      if (has) {
        const uint32_t pos = pre + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const uint32_t w = winner[j];
        const Candidate c = part_cands(parts, part_bytes, w / cap, L)[w % cap];
        ms_qfeat[pos] = j;
        ms_landmark[pos] = c.landmark_id;
        const float2 kp = q_kpt[j];
        double ux = (double)kp.x, uy = (double)kp.y;  // cam_I->get_ud_pixel(qFeatLoc[j])   localization.cpp:484-487
        if (radial_k3) ud_pixel_k3(f, ppx, ppy, k1, k2, k3, ux, uy, &ux, &uy);
        pt2d[2 * pos] = ux;
        pt2d[2 * pos + 1] = uy;
        pt3d[3 * pos] = c.X[0];
        pt3d[3 * pos + 1] = c.X[1];
        pt3d[3 * pos + 2] = c.X[2];
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < 16; ++w) t += wave_cnt[w];
        base_s += t;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) *ms_n = base_s;
    // K5's initial state, normalised points and logcombi tables for the base_s correspondences just written
    __shared__ double s_terms[kP3pMaxN / 2 + 1];
    __syncthreads();
    p3p_init_block(init, (int)base_s, 1024, s_terms);
  }
};
__global__ __launch_bounds__(1024) void k_match_set_finish(const unsigned char *parts, uint32_t n_parts,
                                                  uint64_t part_bytes,
                                                  uint32_t cap, const unsigned long long *best,
                                                  uint32_t *winner, uint32_t nq, const float2 *q_kpt,
                                                  uint32_t *ms_n, uint32_t *ms_qfeat, uint32_t *ms_landmark,
                                                  double *pt2d, double *pt3d, int radial_k3, double f, double ppx,
                                                  double ppy, double k1, double k2, double k3, PartLayout L,
                                                  P3pArgs init /*K5's start, by this workgroup: one launch less*/) {
  MatchSetFinishBody::run(parts, n_parts, part_bytes, cap, best, winner, nq, q_kpt, ms_n, ms_qfeat, ms_landmark, pt2d, pt3d,
                          radial_k3, f, ppx, ppy, k1, k2, k3, L, init);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int launch_emit_candidates(Ctx *c, const Query *q, const QueryPass &pass, uint32_t n_sel, bool all_views) {
  Map *m = c->map;
  if (!pass.cleared) {
    SFM_RC(c->d_cand_part.zero(kPartHeaderBytes, c->stream));
    SFM_RC(dev_zero(c->d_view_stats, 3, c->stream));
    SFM_RC(c->d_best64.fill(0xFF, (size_t)(q->n ? q->n : 1), c->stream));
  }
  if (n_sel == 0 || q->n == 0) return SFMLOC_OK;
  const uint32_t *sel = all_views ? nullptr : c->d_view_sel;
  const uint32_t *gj = c->geo_is_pairs ? c->d_geo_j : nullptr;
  SFM_RC(sfm_launch<EmitMinBody>(c, k_emit_min, dim3(n_sel), dim3(256), 0, sel, n_sel, m->d_view_off, m->d_view_id,
                                 c->d_view_count, c->d_match_i, c->d_match_key, c->d_geo_count, c->d_geo_idx, gj,
                                 m->d_row_landmark, c->d_best64, c->d_geo_dist, (uint32_t)m->params.min_putative,
                                 c->d_view_stats));
  return sfm_launch<EmitWinBody>(c, k_emit_win, dim3(n_sel), dim3(256), 0, sel, n_sel, m->d_view_off, m->d_view_id,
                                 c->d_match_i, c->d_match_key, c->d_geo_count, c->d_geo_idx, gj, m->d_row_landmark,
                                 m->d_landmark_id, m->d_landmark_X, c->d_best64, c->d_geo_dist,
                                 reinterpret_cast<Candidate *>(c->d_cand_part + kPartHeaderBytes), c->cand_cap,
                                 reinterpret_cast<uint32_t *>(c->d_cand_part.get()), c->d_status);
}

// a context's candidate part -> a caller's buffer: the 16-byte header (true count) and the candidates that exist, at
// most cap of them (a fixed-size copy would move cap * 40 bytes for a few hundred candidates)
struct ExportPartBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst,
                                             uint32_t cap) {
    const uint32_t n = min(*reinterpret_cast<const uint32_t *>(src), cap);
    const uint64_t words = (kPartHeaderBytes + (uint64_t)n * sizeof(Candidate)) / 8;  // both multiples of 8
    const uint2 *s8 = reinterpret_cast<const uint2 *>(src);
    uint2 *d8 = reinterpret_cast<uint2 *>(dst);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x)
      d8[i] = s8[i];
  }
};
__global__ __launch_bounds__(256) void k_export_part(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst,
                                             uint32_t cap) {
  ExportPartBody::run(src, dst, cap);
}

int launch_export_part(Ctx *c, void *dst_dev, uint32_t cap) {
  return sfm_launch<ExportPartBody>(c, k_export_part, dim3(8), dim3(256), 0, c->d_cand_part,
                                    reinterpret_cast<unsigned char *>(dst_dev), cap);
}

// a context's candidates appended to a batch's packed part (layout: PartLayout above).  One workgroup: lane 0 claims
// [off, off + n) of the candidate area with one atomic on the header's running total, then everybody copies.
struct ExportPackedBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const unsigned char *__restrict__ src, uint32_t src_cap,
                                               unsigned char *__restrict__ dst, uint32_t n_queries,
                                               uint32_t budget, uint32_t qi) {
    __shared__ uint32_t s_off, s_n;
    uint32_t *h = reinterpret_cast<uint32_t *>(dst);
    if (threadIdx.x == 0) {
      const uint32_t n_true = *reinterpret_cast<const uint32_t *>(src);
      const uint32_t n = min(n_true, src_cap);
      if (n_true > src_cap) atomicOr(&h[3], 2u);      // the context itself overflowed: candidates are lost
      const uint32_t off = atomicAdd(&h[0], n);       // the total keeps counting past the budget: every rank sees by how much
      const bool fits = (uint64_t)off + n <= budget;
      if (!fits) atomicOr(&h[3], 1u);
      h[1] = n_queries;
      h[2] = budget;
      h[4 + qi] = fits ? n : 0u;
      h[4 + n_queries + qi] = fits ? off : 0u;
      s_off = off;
      s_n = fits ? n : 0u;
    }
    __syncthreads();
    const uint2 *s8 = reinterpret_cast<const uint2 *>(src + kPartHeaderBytes);
    uint2 *d8 = reinterpret_cast<uint2 *>(dst + packed_cands_offset(n_queries) + (uint64_t)s_off * sizeof(Candidate));
    const uint64_t words = (uint64_t)s_n * (sizeof(Candidate) / 8);
    for (uint64_t i = threadIdx.x; i < words; i += blockDim.x) d8[i] = s8[i];
  }
};
__global__ __launch_bounds__(256) void k_export_packed(const unsigned char *__restrict__ src, uint32_t src_cap,
                                               unsigned char *__restrict__ dst, uint32_t n_queries,
                                               uint32_t budget, uint32_t qi) {
  ExportPackedBody::run(src, src_cap, dst, n_queries, budget, qi);
}

uint64_t packed_part_bytes(uint32_t n_queries, uint32_t budget) {
  return packed_cands_offset(n_queries) + (uint64_t)budget * sizeof(Candidate);
}

int launch_export_packed(Ctx *c, void *dst_dev, uint32_t n_queries, uint32_t budget, uint32_t qi) {
  return sfm_launch<ExportPackedBody>(c, k_export_packed, dim3(1), dim3(256), 0, c->d_cand_part, c->cand_cap,
                                      reinterpret_cast<unsigned char *>(dst_dev), n_queries, budget, qi);
}

// what a query's 2D-3D selection starts from when no k_query_reset ran for it (sfmloc_merge_begin, the staged API)
struct SelectResetBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(unsigned long long *__restrict__ best64, uint32_t nq, uint32_t *__restrict__ ms_n,
                                             int *__restrict__ status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nq) best64[i] = ~0ull;
    if (i == 0) {
      *ms_n = 0;
      if (status) *status = 0;
    }
  }
};
__global__ __launch_bounds__(256) void k_select_reset(unsigned long long *__restrict__ best64, uint32_t nq,
                                                      uint32_t *__restrict__ ms_n, int *__restrict__ status) {
  SelectResetBody::run(best64, nq, ms_n, status);
}

int launch_select_candidates(Ctx *c, const Query *q, const QueryPass &pass, const unsigned char *parts, uint32_t n_parts,
                             uint64_t part_bytes, uint32_t cap, uint32_t packed_b, uint32_t packed_qi, bool reset_status) {
  PartLayout L;
  L.packed_b = packed_b;
  L.qi = packed_qi;
  if (!pass.cleared) {  // (one launch, and one that a gang session can carry, instead of three memsets)
    const uint32_t nq1 = q->n ? q->n : 1;
    SFM_RC(sfm_launch<SelectResetBody>(c, k_select_reset, dim3((nq1 + 255) / 256), dim3(256), 0, c->d_best64, nq1,
                                       c->d_ms_n, reset_status ? c->d_status : nullptr));
  }
  if (q->n == 0 || n_parts == 0) return SFMLOC_OK;
  const dim3 grid(16, n_parts < 64 ? n_parts : 64);
  // the context's own part (single GPU: the emission just ran on this stream) already holds exactly the winners and
  // d_best64 their keys, so the minimum pass would change nothing
  const bool own_part = (parts == c->d_cand_part && n_parts == 1 && packed_b == 0 && pass.cleared);
  if (!own_part) {
    SFM_RC(sfm_launch<CandidatesMinBody>(c, k_candidates_min, grid, dim3(256), 0, parts, n_parts, part_bytes, cap, q->n,
                                         c->d_best64, c->d_status, L));
  }
  SFM_RC(sfm_launch<MatchSetFinishBody>(c, k_match_set_finish, dim3(1), dim3(1024), 0, parts, n_parts, part_bytes, cap,
                                        c->d_best64, c->d_winner, q->n, q->d_kpt, c->d_ms_n, c->d_ms_qfeat,
                                        c->d_ms_landmark, c->d_pt2d, c->d_pt3d,
                                        (c->map->intrinsic_type == 3 && !c->p3p_uncal) ? 1 : 0, c->map->focal,
                                        c->map->ppx, c->map->ppy, c->map->k1, c->map->k2, c->map->k3, L,
                                        make_p3p_args(c, k5_in(c))));
  c->p3p_init_fused = true;  // launch_p3p_init is then a no-op for this query
  return SFMLOC_OK;
}

int launch_match_set(Ctx *c, const Query *q, const QueryPass &pass, uint32_t n_sel, bool all_views) {
  int rc = launch_emit_candidates(c, q, pass, n_sel, all_views);
  if (rc) return rc;
  return launch_select_candidates(c, q, pass, c->d_cand_part, 1, kPartHeaderBytes + (uint64_t)c->cand_cap * sizeof(Candidate),
                                  c->cand_cap);
}
}  // namespace sfmloc
