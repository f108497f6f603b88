// sfmloc_tracks: feature tracks from pairwise matches (OpenMVG's TracksBuilder::Build + Filter), the first half of
// openMVG_main_ComputeStructureFromKnownPoses.  The semantics are stated in include/sfmloc.h ("sfmloc_tracks"); the
// kernels below name the paragraph they implement.
//
//   components  every match is an edge between two global feature rows; the hook and pointer-jump passes of
//               graph_device.h, repeated until one hooks nothing: a root is the smallest row of its component.
//   order       the touched rows are compacted in ascending row (a scan, no atomic decides a position) and sorted by
//               label with the stable radix sort of radix_sort.h: components ascend by label, rows ascend inside one.
//   filter      two neighbours of one component in the same view are a conflict (rows of a view are contiguous, so
//               two features of one view are neighbours after the sort); flags by atomicOr, counts by atomicAdd on
//               integers.  Track ids and offsets are exclusive scans over the kept components.
// The result is read back once and kept on the host: its consumer, sfmloc_sfm_create, takes host arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "graph_device.h"
#include "radix_sort.h"
#include "sfmloc_internal.h"
#include "tracks_host.h"

namespace sfmloc {
namespace {

thread_local double g_tracks_last_ms = 0.0;

struct Tracks {
  uint64_t counts[4] = {0, 0, 0, 0};  // components, dropped for conflict, dropped for length, kept
  std::vector<uint64_t> off;          // [n_tracks + 1]
  std::vector<uint32_t> view, feat;   // [off[n_tracks]]
};

__global__ __launch_bounds__(256) void k_trk_init(uint32_t *__restrict__ parent, uint32_t *__restrict__ touched,
                                                  uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = i;
  if (i <= n) touched[i] = 0;  // (entry n: where the scan leaves the total)
}

// (every writer stores the same 1)
__global__ __launch_bounds__(256) void k_trk_mark(const uint32_t *__restrict__ ea, const uint32_t *__restrict__ eb,
                                                  uint32_t m, uint32_t *__restrict__ touched) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  touched[ea[e]] = 1;
  touched[eb[e]] = 1;
}

// ---- exclusive scan of a[0..n) in place over several workgroups: per-block scan + block totals, the totals scanned by
// radix_sort.h's one-workgroup k_scan_excl, then added back
__global__ __launch_bounds__(1024) void k_trk_scan_block(uint32_t *__restrict__ a, uint32_t n, uint32_t *__restrict__ sums) {
  __shared__ uint32_t s[1024];
  const int t = threadIdx.x;
  const uint32_t i = blockIdx.x * 1024u + t;
  const uint32_t v = i < n ? a[i] : 0u;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t x = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  if (i < n) a[i] = s[t] - v;
  if (t == 1023) sums[blockIdx.x] = s[1023];
}
__global__ __launch_bounds__(1024) void k_trk_scan_add(uint32_t *__restrict__ a, uint32_t n, const uint32_t *__restrict__ sums) {
  const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
  if (i < n) a[i] += sums[blockIdx.x];
}

// the touched rows in ascending row with their labels (pos = the scanned touched flags, [n + 1])
__global__ __launch_bounds__(256) void k_trk_compact(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ parent,
                                                     uint32_t n, uint32_t *__restrict__ key, uint32_t *__restrict__ node) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || pos[i + 1] == pos[i]) return;
  key[pos[i]] = parent[i];
  node[pos[i]] = i;
}

// head[p] = 1 where a component starts in the sorted list; head[m] = 0 (where the scan leaves the component count)
__global__ __launch_bounds__(256) void k_trk_heads(const uint32_t *__restrict__ key, uint32_t m, uint32_t *__restrict__ head) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p > m) return;
  head[p] = (p < m && (p == 0 || key[p] != key[p - 1])) ? 1u : 0u;
}

// the view of a global feature row: the last v with view_off[v] <= row (views without features share an offset)
__device__ __forceinline__ uint32_t trk_view_of(const uint32_t *__restrict__ view_off, uint32_t n_views, uint32_t row) {
  uint32_t lo = 0, hi = n_views;  // view_off[lo] <= row < view_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (view_off[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

// sfmloc.h "filter": where every component starts, and whether two of its rows lie in one view.  ex = the scanned head
// flags [m + 1]: position p belongs to component ex[p + 1] - 1.  conf is zero on entry.
__global__ __launch_bounds__(256) void k_trk_components(const uint32_t *__restrict__ key, const uint32_t *__restrict__ node,
                                                        const uint32_t *__restrict__ ex, uint32_t m,
                                                        const uint32_t *__restrict__ view_off, uint32_t n_views,
                                                        uint32_t *__restrict__ start, uint32_t *conf) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const uint32_t c = ex[p + 1] - 1;
  if (ex[p + 1] != ex[p]) start[c] = p;
  if (p == m - 1) start[c + 1] = m;
  if (p > 0 && key[p] == key[p - 1] &&
      trk_view_of(view_off, n_views, node[p]) == trk_view_of(view_off, n_views, node[p - 1]))
    atomicOr(conf + c, 1u);
}

// kept[c] = 1 / size[c] = its rows for a component that stays, 0 / 0 otherwise; entry n_comp = 0 (the scans' totals);
// counts: conflict, length, kept
__global__ __launch_bounds__(256) void k_trk_filter(const uint32_t *__restrict__ start, const uint32_t *__restrict__ conf,
                                                    uint32_t n_comp, uint32_t min_length, uint32_t *__restrict__ kept,
                                                    uint32_t *__restrict__ size, uint32_t *counts) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c > n_comp) return;
  uint32_t k = 0, sz = 0;
  if (c < n_comp) {
    sz = start[c + 1] - start[c];
    if (conf[c]) atomicAdd(counts + 0, 1u);
    else if (sz < min_length) atomicAdd(counts + 1, 1u);
    else {
      atomicAdd(counts + 2, 1u);
      k = 1;
    }
  }
  kept[c] = k;
  size[c] = k ? sz : 0u;
}

// sfmloc.h "order": the rows of the kept components as (view, feature), track t at toff[c] .. ; tid / toff = the scanned
// kept flags and sizes [n_comp + 1]
__global__ __launch_bounds__(256) void k_trk_emit(const uint32_t *__restrict__ node, const uint32_t *__restrict__ ex,
                                                  uint32_t m, const uint32_t *__restrict__ start,
                                                  const uint32_t *__restrict__ tid, const uint32_t *__restrict__ toff,
                                                  const uint32_t *__restrict__ view_off, uint32_t n_views,
                                                  uint32_t *__restrict__ out_off, uint32_t *__restrict__ out_view,
                                                  uint32_t *__restrict__ out_feat) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const uint32_t c = ex[p + 1] - 1;
  if (tid[c + 1] == tid[c]) return;
  const uint32_t at = toff[c] + (p - start[c]);
  const uint32_t row = node[p], v = trk_view_of(view_off, n_views, row);
  out_view[at] = v;
  out_feat[at] = row - view_off[v];
  if (p == start[c]) out_off[tid[c]] = toff[c];
}

int scan_excl(uint32_t *a, uint32_t n, uint32_t *sums, hipStream_t s) {
  const uint32_t nb = (n + 1023) / 1024;
  SFM_RC(dev_launch(k_trk_scan_block, dim3(nb), dim3(1024), 0, s, a, n, sums));
  SFM_RC(dev_launch(k_scan_excl, dim3(1), dim3(1024), 0, s, sums, nb));
  return dev_launch(k_trk_scan_add, dim3(nb), dim3(1024), 0, s, a, n, sums);
}

int read_u32(uint32_t *out, const uint32_t *d, hipStream_t s) {
  SFM_RC(dev_download(out, d, 1, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

int tracks_device(const uint64_t *view_off64, uint32_t n_views, uint32_t n, const std::vector<uint32_t> &ea,
                  const std::vector<uint32_t> &eb, uint32_t min_length, hipStream_t s, Tracks *t) {
  const uint32_t m_edges = (uint32_t)ea.size();
  std::vector<uint32_t> voff((size_t)n_views + 1);
  for (uint32_t v = 0; v <= n_views; ++v) voff[v] = (uint32_t)view_off64[v];
  DevBuf<uint32_t> d_voff, d_ea, d_eb, d_parent, d_touched, d_sums, d_flag;
  SFM_RC(d_voff.alloc(nullptr, voff.size()));
  SFM_RC(d_ea.alloc(nullptr, m_edges));
  SFM_RC(d_eb.alloc(nullptr, m_edges));
  SFM_RC(d_parent.alloc(nullptr, n));
  SFM_RC(d_touched.alloc(nullptr, (size_t)n + 1));
  SFM_RC(d_sums.alloc(nullptr, (size_t)n / 1024 + 2));
  SFM_RC(d_flag.alloc(nullptr, 4));  // changed, then the three counts of the filter
  SFM_RC(d_voff.upload(voff.data(), voff.size(), s));
  SFM_RC(d_ea.upload(ea.data(), m_edges, s));
  SFM_RC(d_eb.upload(eb.data(), m_edges, s));
  const dim3 gn((n + 1 + 255) / 256), ge((m_edges + 255) / 256), b256(256);
  SFM_RC(dev_launch(k_trk_init, gn, b256, 0, s, d_parent, d_touched, n));
  SFM_RC(dev_launch(k_trk_mark, ge, b256, 0, s, d_ea, d_eb, m_edges, d_touched));
  for (;;) {  // sfmloc.h "components": until a pass hooks nothing
    SFM_RC(d_flag.zero(1, s));
    SFM_RC(dev_launch(k_graph_hook, ge, b256, 0, s, d_ea, d_eb, m_edges, d_parent, d_flag));
    SFM_RC(dev_launch(k_graph_jump, gn, b256, 0, s, d_parent, n));
    uint32_t changed = 0;
    SFM_RC(read_u32(&changed, d_flag, s));
    if (!changed) break;
  }
  d_ea.reset();
  d_eb.reset();
  // the touched rows, ascending, with their labels
  SFM_RC(scan_excl(d_touched, n + 1, d_sums, s));
  uint32_t m = 0;
  SFM_RC(read_u32(&m, d_touched.get() + n, s));
  DevBuf<uint32_t> d_key, d_node, d_key2, d_node2, d_hist, d_ex;
  SFM_RC(d_key.alloc(nullptr, m));
  SFM_RC(d_node.alloc(nullptr, m));
  SFM_RC(d_key2.alloc(nullptr, m));
  SFM_RC(d_node2.alloc(nullptr, m));
  SFM_RC(d_hist.alloc(nullptr, radix_hist_entries(m)));
  SFM_RC(d_ex.alloc(nullptr, (size_t)m + 1));
  SFM_RC(dev_launch(k_trk_compact, gn, b256, 0, s, d_touched, d_parent, n, d_key, d_node));
  bool swapped = false;
  SFM_RC(radix_sort_pairs(d_key, d_node, d_key2, d_node2, m, radix_key_bits(n - 1), d_hist, s, &swapped));
  const uint32_t *key = swapped ? d_key2.get() : d_key.get(), *node = swapped ? d_node2.get() : d_node.get();
  const dim3 gm((m + 1 + 255) / 256);
  SFM_RC(dev_launch(k_trk_heads, gm, b256, 0, s, key, m, d_ex));
  SFM_RC(scan_excl(d_ex, m + 1, d_sums, s));
  uint32_t n_comp = 0;
  SFM_RC(read_u32(&n_comp, d_ex.get() + m, s));
  d_parent.reset();
  d_touched.reset();
  DevBuf<uint32_t> d_start, d_conf, d_tid, d_toff;
  SFM_RC(d_start.alloc(nullptr, (size_t)n_comp + 1));
  SFM_RC(d_conf.alloc(nullptr, n_comp));
  SFM_RC(d_tid.alloc(nullptr, (size_t)n_comp + 1));
  SFM_RC(d_toff.alloc(nullptr, (size_t)n_comp + 1));
  SFM_RC(d_conf.zero(n_comp, s));
  SFM_RC(d_flag.zero(4, s));
  SFM_RC(dev_launch(k_trk_components, gm, b256, 0, s, key, node, d_ex, m, d_voff, n_views, d_start, d_conf));
  SFM_RC(dev_launch(k_trk_filter, dim3((n_comp + 1 + 255) / 256), b256, 0, s, d_start, d_conf, n_comp, min_length,
                    d_tid, d_toff, d_flag.get() + 1));
  SFM_RC(scan_excl(d_tid, n_comp + 1, d_sums, s));
  SFM_RC(scan_excl(d_toff, n_comp + 1, d_sums, s));
  uint32_t n_tracks = 0, n_rows = 0, cnt[4] = {0, 0, 0, 0};
  SFM_RC(d_flag.download(cnt, 4, s));
  SFM_RC(read_u32(&n_tracks, d_tid.get() + n_comp, s));
  SFM_RC(read_u32(&n_rows, d_toff.get() + n_comp, s));
  DevBuf<uint32_t> d_off, d_view, d_feat;
  SFM_RC(d_off.alloc(nullptr, n_tracks));
  SFM_RC(d_view.alloc(nullptr, n_rows));
  SFM_RC(d_feat.alloc(nullptr, n_rows));
  SFM_RC(dev_launch(k_trk_emit, gm, b256, 0, s, node, d_ex, m, d_start, d_tid, d_toff, d_voff, n_views, d_off, d_view,
                    d_feat));
  std::vector<uint32_t> off32(n_tracks);
  t->view.resize(n_rows);
  t->feat.resize(n_rows);
  if (n_tracks) SFM_RC(d_off.download(off32.data(), n_tracks, s));
  if (n_rows) {
    SFM_RC(d_view.download(t->view.data(), n_rows, s));
    SFM_RC(d_feat.download(t->feat.data(), n_rows, s));
  }
  SFM_HIP(hipStreamSynchronize(s));
  t->off.assign(off32.begin(), off32.end());
  t->off.push_back(n_rows);
  t->counts[0] = n_comp;
  t->counts[1] = cnt[1];
  t->counts[2] = cnt[2];
  t->counts[3] = cnt[3];
  return SFMLOC_OK;
}

int tracks_build_impl(int device, const PairScene &sc, const uint8_t *view_use, uint32_t min_length, Tracks *t) {
  std::vector<uint32_t> ea, eb;
  uint64_t n_nodes = 0;
  std::string err;
  const int rc = tracks_host::flatten(sc, view_use, &ea, &eb, &n_nodes, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  t->off.assign(1, 0);
  // (no match: no track, nothing to launch)
  return timed_call(device, &g_tracks_last_ms, !ea.empty() && n_nodes != 0, [&](hipStream_t s) {
    return tracks_device(sc.view_off, sc.n_views, (uint32_t)n_nodes, ea, eb, min_length < 1 ? 1 : min_length, s, t);
  });
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

int sfmloc_tracks_build(int device, const uint64_t *view_off, uint32_t n_views, const uint8_t *view_use,
                        const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets, const uint32_t *match_i,
                        const uint32_t *match_j, uint32_t min_length, sfmloc_tracks **out) {
  PairScene sc{};  // (the views' offsets and the pair list: tracks know nothing of the cameras)
  sc.view_off = view_off, sc.n_views = n_views, sc.pairs = pairs, sc.n_pairs = n_pairs, sc.offsets = offsets;
  sc.match_i = match_i, sc.match_j = match_j;
  return make_handle<Tracks>("sfmloc_tracks_build", out,
                             [&](Tracks *t) { return tracks_build_impl(device, sc, view_use, min_length, t); });
}

int sfmloc_tracks_counts(const sfmloc_tracks *tt, uint64_t *counts) {
  SFM_CHECK(tt && counts, SFMLOC_EINVAL, "sfmloc_tracks_counts: null argument");
  memcpy(counts, reinterpret_cast<const Tracks *>(tt)->counts, 4 * sizeof(uint64_t));
  return SFMLOC_OK;
}

int sfmloc_tracks_read(const sfmloc_tracks *tt, uint64_t *off, uint32_t *view, uint32_t *feat) {
  SFM_CHECK(tt, SFMLOC_EINVAL, "sfmloc_tracks_read: null handle");
  const Tracks *t = reinterpret_cast<const Tracks *>(tt);
  if (off) memcpy(off, t->off.data(), t->off.size() * sizeof(uint64_t));
  if (view && !t->view.empty()) memcpy(view, t->view.data(), t->view.size() * sizeof(uint32_t));
  if (feat && !t->feat.empty()) memcpy(feat, t->feat.data(), t->feat.size() * sizeof(uint32_t));
  return SFMLOC_OK;
}

void sfmloc_tracks_destroy(sfmloc_tracks *t) { delete reinterpret_cast<Tracks *>(t); }

double sfmloc_tracks_last_ms(void) { return g_tracks_last_ms; }

}  // extern "C"
