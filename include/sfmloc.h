/*
 * sfmloc.h -- C ABI of the MI355X-native query-localisation hot path.
 *
 * This is the drop-in boundary for ONE path of hulop/SfMLocalization: what
 * OpenMVGLocalization_AKAZE's per-query loop (reference
 * OpenMVGLocalization_AKAZE/src/localization.cpp:285-586) and its in-process
 * twin LocalizeEngine::localize (VisionLocalizeServer/src/LocalizeEngine.cc:288-661)
 * do between "query descriptors are known" and "pose is known".
 * The reference has no FFI for this path (it is a CLI + files, or a C++ class);
 * the entry points below are what a binding for it would call.  Each one
 * cites the reference interface it replaces.
 *
 * Conventions
 *   - plain C, opaque handles, caller-owned output buffers, no torch types;
 *   - every function returns an int status: 0 = ok, <0 = error, text via
 *     sfmloc_last_error() (thread local);
 *   - "localisation failed" is NOT an error: status 0 with n_inliers == 0
 *     (reference: failure JSON without "t", localization.cpp:419-446,511-542);
 *   - one handle = one map (or one shard of a map) on one GPU; calls on one
 *     handle are serialised by the caller (the reference object is not
 *     re-entrant either, LocalizeEngine.cc:398-399,627-628);
 *   - there is no CPU fallback: without a HIP device every compute entry point
 *     returns SFMLOC_ENODEV.
 */
#ifndef SFMLOC_H
#define SFMLOC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFMLOC_ABI_VERSION 2   /* 2: sfmloc_params.guided_matching */
#define SFMLOC_DESC_BYTES 64          /* FileUtils.cpp:77-92: 61 M-LDB bytes + 3 zero bytes */
#define SFMLOC_NOMATCH 0xFFFFFFFFu
#define SFMLOC_MAX_QUERY_ROWS 65535u  /* query feature index is packed into 16 bits of the match key */

enum {
  SFMLOC_OK = 0,
  SFMLOC_EINVAL = -1, /* bad argument / shape */
  SFMLOC_ENODEV = -2, /* no HIP device: the product path has no CPU fallback */
  SFMLOC_EHIP = -3,   /* HIP runtime error */
  SFMLOC_EIO = -4,    /* file contract violated */
  SFMLOC_ECAP = -5,   /* caller buffer too small */
  SFMLOC_ENOMEM = -6
};

const char *sfmloc_last_error(void);
int sfmloc_abi_version(void);
/* number of HIP devices visible (0 on a CPU-only box); never fails */
int sfmloc_device_count(void);

/* ------------------------------------------------------------------------- */
/* Parameters: the reference's CLI keys (localization.cpp:64-82) and its      */
/* compile-time constants (localization.cpp:56-58).                            */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_params {
  float dist_ratio;         /* -f fDistRatio, default 0.6 */
  int ransac_round;         /* -r ransacRound (F-matrix AC-RANSAC iterations), default 200; callers pass 25 */
  double geom_precision;    /* -g geomLimit, default 4.0 px */
  int bow_knn;              /* -k knnbow, 0 = no shortlist.  Recorded with the map for the callers (the command-line tools
                             * and engine mirrors read it back); the library itself takes the shortlist length as an
                             * argument of sfmloc_bow_select / sfmloc_localize_bow_begin, because the reference decides it
                             * per call (LocalizeEngine.cc:337-340: only when the map has more views than knn) */
  int min_putative;         /* MINUM_NUMBER_OF_POINT_PUTATIVE_MATCH = 16 */
  int min_resection_points; /* MINUM_NUMBER_OF_POINT_RESECTION = 8 (test is ">") */
  int min_inliers;          /* MINUM_NUMBER_OF_INLIER_RESECTION = 10 (test is ">") */
  int p3p_max_iteration;    /* OpenMVG Image_Localizer_Match_Data::max_iteration default 4096 */
  uint64_t seed;            /* counter-based RNG seed (the reference's RNG is unseeded) */
  int refine_pose;          /* north-star extension A13; 0 = reference-equivalent output */
  int device;               /* HIP device ordinal */
  int profile;              /* 1 = bracket each stage with HIP events on the handle's stream, 2 = the Hamming scan only */
  int exact_rows;           /* 1 = keep the exact (nearest, second) pair of EVERY bank row (sfmloc_putative_read_rows);
                               0 = rows the screening kernel proves rejected are not finished (same matches) */
  int guided_matching;      /* -gm guidedMatch (localization.cpp:82,183; computeFeaturesAndMatches.cpp:63,89; the map
                               builder's default, ReconstructParam.py:71): every pair that passes the F-matrix AC-RANSAC
                               has its matches replaced by OpenMVG's Geometry_guided_matching under the estimated F
                               (MatchUtils.cpp:413-415) */
  int k1_mfma;              /* 1 (default) = unsliced scans of a view list (every shortlist scan while the GPU is shared,
                               long view lists) take their Hamming distances from the matrix cores
                               (k_hamming_screen_mfma: e2m1 +-1 operands, exact); 0 = the popcount form
                               (k_hamming_screen_shortlist).  Same matches either way; the full-bank scan, the sliced
                               scan of a lone query, short queries and exact_rows = 1 are popcount in both settings.
                               (The field occupies what was tail padding of the struct: size and the offsets of the
                               other fields are those of ABI version 2.) */
} sfmloc_params;

void sfmloc_default_params(sfmloc_params *p);

/* ------------------------------------------------------------------------- */
/* Map (= what the reference loads once: localization.cpp:238-280).            */
/* Host arrays are copied to HBM; the caller may free them after the call.     */
/* Views are the reconstruction's images in ascending view id; their           */
/* descriptors are the rows [view_off[v], view_off[v+1]) of the bank, in .desc */
/* file order (FileUtils.cpp:94-103).                                          */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_map_desc {
  uint32_t n_views;
  const uint32_t *view_id;      /* [n_views] strictly ascending */
  const uint32_t *view_off;     /* [n_views+1] row offsets, view_off[0] = 0 */
  const uint32_t *view_wh;      /* [n_views*2] image width,height (sfm_data views) or NULL */
  uint64_t n_rows;              /* = view_off[n_views] */
  const uint8_t *desc;          /* [n_rows*64] .desc payload rows */
  const float *kpt_xy;          /* [n_rows*2] .feat x,y or NULL (needed from the F-matrix stage on) */
  const int32_t *row_landmark;  /* [n_rows] landmark slot of (view,feat) or -1, or NULL */
  uint32_t n_landmarks;
  const uint32_t *landmark_id;  /* [n_landmarks] structure keys */
  const double *landmark_X;     /* [n_landmarks*3] */
  /* intrinsic id 0 (localization.cpp:484-487): pinhole or pinhole_radial_k3 */
  double focal, ppx, ppy, k1, k2, k3;
  uint32_t bow_dim;             /* 0 = no BoW */
  const float *bow;             /* [n_views*bow_dim] .bow vectors as f32 (BoFUtils.cpp:43-45) or NULL */
  /* 0 = pinhole: pt2D = the query keypoint (get_ud_pixel is the identity); 3 = pinhole_radial_k3: pt2D =
   * cam2ima(remove_disto(ima2cam(p))) with (k1, k2, k3) (localization.cpp:484-487).  A radial camera with zero
   * coefficients still goes through remove_disto's bisection, so the type is explicit. */
  uint32_t intrinsic_type;
} sfmloc_map_desc;

typedef struct sfmloc_map sfmloc_map;

/* replaces: Load(sfm_data) + structureToMapViewFeatTo3D + HuloSfMRegionsProvider::load
 * (localization.cpp:238-248,274-280), fed from memory */
int sfmloc_map_create(const sfmloc_map_desc *desc, const sfmloc_params *params, sfmloc_map **out);
void sfmloc_map_destroy(sfmloc_map *map);

/* replaces the same start-up sequence fed from disk: <sfm_dir>/sfm_data.json (cereal JSON: views, intrinsic 0,
 * extrinsics, structure) and <match_dir>/<basename>.{desc,feat[,bow]} of every view that has a pose
 * (localization.cpp:236-280,337-341; file layouts: SURVEY.md Appendix A).  Error text follows the reference's
 * ("The input sfm_data.json file ... cannot be read.").  SFMLOC_EIO when the contract is violated. */
int sfmloc_open(const char *sfm_dir, const char *match_dir, const sfmloc_params *params, sfmloc_map **out);

/* Host-only half of sfmloc_open (no GPU needed): parses the same files and reports what it found. */
typedef struct sfmloc_scan_info {
  uint32_t n_views_total, n_views_posed;
  uint64_t n_rows;
  uint32_t n_landmarks, n_observations, bow_dim;
  double focal, ppx, ppy, k1, k2, k3;
  uint64_t desc_fnv1a;     /* FNV-1a over all descriptor bytes in bank order */
  double kpt_sum;          /* sum of all keypoint coordinates */
  int64_t row_landmark_sum;
} sfmloc_scan_info;
int sfmloc_scan(const char *sfm_dir, const char *match_dir, sfmloc_scan_info *info);

/* Packed map file: everything sfmloc_open reads from sfm_data.json and the per-view .desc / .feat / .bow
 * files, as ONE binary written once by sfmloc_pack (host only) -- a server then opens a 10 000-view map at disk speed
 * instead of parsing a large JSON and 20 000 small files.  sfmloc_open_packed(path) gives the same map as
 * sfmloc_open(sfm_dir, match_dir); sfmloc_scan_packed is the host-only check (same fields as sfmloc_scan).  The file
 * is little-endian and versioned by its 8-byte magic; SFMLOC_EIO for anything else. */
int sfmloc_pack(const char *sfm_dir, const char *match_dir, const char *out_path);
int sfmloc_scan_packed(const char *path, sfmloc_scan_info *info);
int sfmloc_open_packed(const char *path, const sfmloc_params *params, sfmloc_map **out);

/* The view table of an sfm_data.json on its own (host only): what ExtFeatAndMatch iterates over before any
 * reconstruction exists (computeFeaturesAndMatches.cpp:118-126, AKAZEOpenCV.cpp:122-131).  Views come in id order
 * (Views is a std::map); image_path = root_path / file name and stays valid until sfmloc_view_list_close. */
typedef struct sfmloc_view_list sfmloc_view_list;
int sfmloc_view_list_open(const char *sfm_data_json, sfmloc_view_list **out, uint32_t *n_views);
int sfmloc_view_list_get(const sfmloc_view_list *list, uint32_t k, uint32_t *view_id, uint32_t *width,
                         uint32_t *height, const char **image_path);
void sfmloc_view_list_close(sfmloc_view_list *list);

/* view table of a map: ids [n_views], row offsets [n_views+1], camera centres [n_views*3] (only for maps opened
 * from sfm_data.json; used for the dead-reckoning restriction getLocalViews, SfMDataUtils.cpp:210-227) */
int sfmloc_map_views(const sfmloc_map *map, uint32_t *view_id, uint32_t *view_off, double *center);
/* image width, height of every view [n_views*2] (sfm_data views; the default size of a query without an image) */
int sfmloc_map_view_sizes(const sfmloc_map *map, uint32_t *wh);

typedef struct sfmloc_map_info {
  uint64_t n_rows;
  uint32_t n_views;
  uint32_t n_landmarks;
  uint64_t hbm_bytes; /* device memory held by the handle */
  int device;
} sfmloc_map_info;
int sfmloc_map_get_info(const sfmloc_map *map, sfmloc_map_info *info);

/* ------------------------------------------------------------------------- */
/* Query (= the output of extractAKAZESingleImg, AKAZEOpenCV.cpp:37-113).      */
/* Uploading it is separate from matching so that callers (and bench.py) can   */
/* have inputs resident in HBM before the timed region.                        */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_query sfmloc_query;

int sfmloc_query_create(sfmloc_map *map, const uint8_t *desc /*[n*64]*/, const float *kpt_xy /*[n*2] or NULL*/,
                        uint32_t n, uint32_t width, uint32_t height, sfmloc_query **out);
void sfmloc_query_destroy(sfmloc_query *q);
/* The query's BoW vector [bow_dim of the map] made resident with the query (what calcBoF produced for it,
 * LocalizeEngine.cc:337-340): sfmloc_localize_bow_begin / sfmloc_shard_bow_keys then take query_bow = NULL and no
 * per-call upload happens.  Synchronous. */
int sfmloc_query_set_bow(sfmloc_query *q, const float *query_bow);
/* Marks the query as taken by a camera nobody calibrated ("Uncalibrated queries" below); on = 0 clears the mark.  The
 * property is the query's, not the map's: the same map serves marked and unmarked queries, also within one batch.  Any
 * query that carries its image size can be marked, one over the caller's device arrays (sfmloc_query_create_view)
 * included. */
int sfmloc_query_set_uncalibrated(sfmloc_query *q, int on);
/* A query over arrays that already ARE in device memory and stay the caller's -- e.g. slices of the buffer an all-gather
 * of extracted features wrote (images in on several ranks: the rank that owns a query extracts it, every rank matches
 * it).  Nothing is allocated or copied; the arrays must stay valid and unchanged while the query is in use.
 *   desc_dev  uint8 [n_pad * 64], row major, n_pad = n rounded up to a multiple of 64, the rows beyond n ZERO; 16-byte aligned
 *   kpt_dev   float [n * 2] as extracted;  kpt6_dev  float [n * 2] after sfmloc_feat_round_trip;  8-byte aligned
 *   bow_dev   float [bow_dim of the map], or NULL (then the calls that need one take a host pointer as usual)
 * sfmloc_feat_round_trip: host helper, the `.feat` text round trip of the keypoints (6 significant digits,
 * AKAZEOpenCV.cpp:80-81 / :106-111) that sfmloc_query_create applies itself. */
int sfmloc_query_create_view(sfmloc_map *map, const void *desc_dev, const void *kpt_dev, const void *kpt6_dev,
                             const void *bow_dev, uint32_t n, uint32_t width, uint32_t height, sfmloc_query **out);
void sfmloc_feat_round_trip(const float *kpt_xy, uint64_t n_values, float *out);

/* ------------------------------------------------------------------------- */
/* Stage A6+A7: putative matching.                                             */
/* replaces hulo::matchAKAZEToQuery (MatchUtils.cpp:283-367) with an exact     */
/* 2-NN in place of the reference's LSH, then the "< 16 matches" filter        */
/* (localization.cpp:408-415).                                                 */
/*   view_sel: indices into the map's view table (NOT view ids), strictly      */
/*   ascending, or NULL for all views (localization.cpp:386-392).              */
/* Results stay on the device for the next stage; sfmloc_putative_read copies  */
/* them out.  Asynchronous on the handle's stream.                             */
/* ------------------------------------------------------------------------- */
int sfmloc_match_putative(sfmloc_map *map, sfmloc_query *q, const uint32_t *view_sel, uint32_t n_sel);

/* Blocks until the stream is idle, then copies out
 *   view_count[n_views]          matches per view (0 for unselected views), BEFORE the >=16 filter
 *   match_i/match_j/match_d[cap] per-view lists, view v's list starting at row offset view_off[v]
 *                                (so cap must be >= n_rows), in ascending map-feature index i.
 * Any pointer may be NULL. */
int sfmloc_putative_read(sfmloc_map *map, uint32_t *view_count, uint32_t *match_i, uint32_t *match_j,
                         uint32_t *match_d, uint64_t cap);

/* Per-row view of the same stage (parity tests): key[r] = (d0<<16)|j0 of the nearest query
 * descriptor and of the second nearest, for every bank row that was searched, SFMLOC_NOMATCH elsewhere. */
int sfmloc_putative_read_rows(sfmloc_map *map, uint32_t *best0 /*[n_rows]*/, uint32_t *best1 /*[n_rows]*/);

int sfmloc_sync(sfmloc_map *map);

/* ------------------------------------------------------------------------- */
/* Stage A8: geometric filter.                                                 */
/* replaces hulo::geometricMatch (MatchUtils.cpp:372-420) = OpenMVG            */
/* GeometricFilter_FMatrix_AC(geomPrec, ransacRound) per (view, query) pair,   */
/* on the result of the last sfmloc_match_putative call; views with fewer than */
/* params.min_putative matches are dropped first (localization.cpp:408-415).   */
/* Query keypoints are the .feat-rounded ones (6 significant digits), map      */
/* keypoints come from the map's .feat (no undistortion: MatchUtils.cpp:381).  */
/* ------------------------------------------------------------------------- */
int sfmloc_geometric_filter(sfmloc_map *map, sfmloc_query *q);
/* geo_count[n_views]; geo_idx[n_rows]: view v's inliers as indices into ITS putative list, stored at
 * view_off[v], in AC-RANSAC's inlier order (ascending residual).  Synchronises. */
int sfmloc_geometric_read(sfmloc_map *map, uint32_t *geo_count, uint32_t *geo_idx, uint64_t cap);
/* The same stage as (map feature i, query feature j) pairs, view v's list at view_off[v]: with guided matching these ARE
 * the result (one match per map feature, ascending i; not a subset of the putative list, so sfmloc_geometric_read
 * refuses), without it the putative matches the indices name.  Synchronises. */
int sfmloc_geometric_read_pairs(sfmloc_map *map, uint32_t *geo_count, uint32_t *geo_i, uint32_t *geo_j, uint64_t cap);

/* ------------------------------------------------------------------------- */
/* Stage A9+A10: 2D-3D match set.                                              */
/* replaces hulo::matchProviderToMatchSet (SfMDataUtils.cpp:59-125) and the    */
/* pt2D/pt3D assembly (localization.cpp:479-501).                              */
/* ------------------------------------------------------------------------- */
int sfmloc_match_set(sfmloc_map *map, sfmloc_query *q);
int sfmloc_match_set_read(sfmloc_map *map, uint32_t *n, uint32_t *qfeat, uint32_t *landmark_id, double *pt2d,
                          double *pt3d, uint32_t cap);

/* ------------------------------------------------------------------------- */
/* Stage A11+A12: resection and pose.                                          */
/* replaces sfm::SfM_Localizer::Localize (localization.cpp:504-509; P3P        */
/* AC-RANSAC, max_iteration = params.p3p_max_iteration), the inlier gate       */
/* (localization.cpp:511) and KRt_From_P / t_out = -R^T t (:544-547).          */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_pose {
  int32_t ok;                /* 1 = localised: what the reference signals by writing "t" into the result JSON */
  int32_t n_inliers;         /* resection_data.vec_inliers.size() */
  int32_t n_matches_2d3d;    /* mapFeatTo3DFeat.size() (cpt, localization.cpp:502) */
  int32_t iterations;        /* AC-RANSAC iterations actually run */
  int32_t status;            /* bit 0/1/2: a capacity of the device workspace was exceeded */
  int32_t n_putative_views;  /* views with >= min_putative matches */
  int32_t n_geometric_views; /* views that passed the F-matrix filter */
  int32_t reserved;
  double nfa;                /* AC-RANSAC minimum NFA (log10) */
  double error_max;          /* resection_data.error_max (pixels) */
  double P[12];              /* projection_matrix, row-major 3x4 */
  double K[9], R[9], t[3];   /* KRt_From_P, row-major */
  double center[3];          /* t_out = -R^T t: the "t" of the result JSON */
  double stage_seconds[7];   /* LocalizeEngine.cc:643-658 buckets: selectBeacon, selectBow, extFeat, putMatch,
                                geoMatch, PnP, others.  Filled from the per-stage HIP events of this query when
                                params.profile == 1 (selectBow = K8, putMatch = K1+K2, geoMatch = K3, PnP = 2D-3D set +
                                P3P, others = the rest of the call's wall time; selectBeacon / extFeat are the caller's);
                                otherwise only others = the call's wall time */
} sfmloc_pose;

int sfmloc_resection(sfmloc_map *map, sfmloc_query *q);
/* pair_*: the "pair" list of the result JSON (localization.cpp:132-141): (query feature, landmark id) per
 * inlier; inlier_idx: indices into the 2D-3D match set.  Synchronises. */
int sfmloc_pose_read(sfmloc_map *map, sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark,
                     uint32_t *inlier_idx, uint32_t cap);

/* The whole per-query path: putative -> >=16 filter -> F-matrix filter -> 2D-3D set -> P3P -> pose
 * (localization.cpp:395-547 / LocalizeEngine.cc:423-585).  One host synchronisation at the end. */
int sfmloc_localize(sfmloc_map *map, sfmloc_query *q, const uint32_t *view_sel, uint32_t n_sel, sfmloc_pose *out,
                    uint32_t *pair_qfeat, uint32_t *pair_landmark, uint32_t cap);

/* Concurrent queries.  A context is a HIP stream plus the workspace of one in-flight query; contexts of one
 * map run concurrently on the GPU (the reference serves concurrent users with one engine per (user, map),
 * localizeImage.cc:71-104 -- here they share one copy of the map).  _begin enqueues the whole path and
 * returns; _end waits for it.  One query per context at a time.  Contexts are owned by the map. */
typedef struct sfmloc_context sfmloc_context;
int sfmloc_context_create(sfmloc_map *map, sfmloc_context **out);
void sfmloc_context_destroy(sfmloc_context *ctx);
int sfmloc_localize_begin(sfmloc_context *ctx, sfmloc_query *q, const uint32_t *view_sel, uint32_t n_sel);
/* localization.cpp:346-368 / LocalizeEngine.cc:333-361 in one asynchronous call: shortlist the `knn` candidate views
 * nearest to `query_bow` (exactly as sfmloc_bow_select) and localise on them.  The shortlist stays on the device --
 * the bank blocks to scan are derived from it by a kernel -- so nothing waits for the host between the two stages.
 * As in the reference the shortlist applies only when more than `knn` candidates remain; cand_views NULL = all
 * views.  query_bow NULL = the vector made resident by sfmloc_query_set_bow.  Finish with sfmloc_localize_end.
 * Same result as sfmloc_bow_select + sfmloc_localize_begin, bit for bit. */
int sfmloc_localize_bow_begin(sfmloc_context *ctx, sfmloc_query *query, const float *query_bow, uint32_t knn,
                              const uint32_t *cand_views, uint32_t n_cand);
/* the same, synchronous, on the map's own context (as sfmloc_localize; the stage read-backs then refer to it) */
int sfmloc_localize_bow(sfmloc_map *map, sfmloc_query *query, const float *query_bow, uint32_t knn,
                        const uint32_t *cand_views, uint32_t n_cand, sfmloc_pose *out, uint32_t *pair_qfeat,
                        uint32_t *pair_landmark, uint32_t cap);
int sfmloc_localize_end(sfmloc_context *ctx, sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark,
                        uint32_t cap);
/* n queries against all views, n_contexts of them in flight (0 = 4).  poses[n]; pair buffers may be NULL,
 * else query i's pairs start at i*pair_stride. */
int sfmloc_localize_batch(sfmloc_map *map, sfmloc_query *const *queries, uint32_t n, uint32_t n_contexts,
                          sfmloc_pose *poses, uint32_t *pair_qfeat, uint32_t *pair_landmark, uint32_t pair_stride);

/* ------------------------------------------------------------------------- */
/* Sharded maps: one process per GPU, each holding a contiguous   */
/* range of views.  Every bank row's decision depends only on the replicated     */
/* query, so putative matching and the F-matrix filter are shard-local; what is   */
/* exchanged is each shard's list of 2D-3D CANDIDATES (a "part": 16-byte header   */
/* {u32 count} + cap 40-byte candidates whose order key carries the global view   */
/* id).  The caller moves parts between ranks (torch.distributed all-gather over  */
/* RCCL) and hands the concatenation to sfmloc_merge_begin, which reproduces      */
/* matchProviderToMatchSet + Localize of the unsharded map bit for bit.           */
/*   dst_dev / parts_dev are DEVICE pointers owned by the caller.                 */
/* ------------------------------------------------------------------------- */
uint64_t sfmloc_part_bytes(uint32_t cap);
int sfmloc_shard_begin(sfmloc_context *ctx, sfmloc_query *q, const uint32_t *view_sel, uint32_t n_sel);
/* writes the part's header (true count) and its first min(count, cap) candidates to dst_dev; bytes beyond are left
 * as they were (the merging side reads `count` entries only) */
int sfmloc_shard_export(sfmloc_context *ctx, void *dst_dev, uint32_t cap);
int sfmloc_context_sync(sfmloc_context *ctx);
/* Ordering against a stream of the caller (e.g. the one its collective runs on) without blocking the host:
 *   _signal: everything queued on the context so far happens before work queued on hip_stream from now on;
 *   _wait:   everything queued on hip_stream so far happens before work queued on the context from now on.
 * hip_stream is a hipStream_t of the same device (NULL = the default stream). */
int sfmloc_context_signal(sfmloc_context *ctx, void *hip_stream);
int sfmloc_context_wait(sfmloc_context *ctx, void *hip_stream);
/* Gang sessions: up to 32 contexts of one map take one query each through the same asynchronous calls
 * (sfmloc_shard_bow_keys, sfmloc_shard_begin[_bow] + sfmloc_shard_export_packed, sfmloc_localize[_bow]_begin), and every
 * kernel of the chain is launched once for all of them (or for as many as its kernel arguments hold: 8 to 32).  Between _begin and _end the calls on these contexts only record
 * their launches; _end issues them -- one launch per kernel, the members side by side in gridDim.z -- on the first
 * context's stream and orders the other members' streams after it.  Results are those of the same calls made one context
 * at a time, bit for bit: a member's arithmetic does not change, only the number of launches (a rank of an N-rank run
 * scans 1/N of the map per query but still issues every query's launches, and the device completes only so many
 * dependent launches per second).  One host thread drives a session; with params.profile != 0 a session records
 * nothing and the members run one after the other.
 *   _counters: launches issued by this leader's sessions so far, and how many of them carried more than one member. */
int sfmloc_gang_begin(sfmloc_context *const *ctxs, uint32_t n);
/* a context (workspace) WITHOUT a stream of its own: its work is queued on `lender`'s stream (a lender destroyed first
 * stops being usable but its stream lives until the last borrower is destroyed).  For
 * the members of a gang other than the first -- a device serves only so many hardware queues well, and a context that
 * only ever works inside gang sessions needs none. */
int sfmloc_context_create_sharing(sfmloc_map *map, sfmloc_context *lender, sfmloc_context **out);
/* a context for sfmloc_merge_begin[_packed] + sfmloc_localize_end ONLY (the owner's stage of a sharded query): none of the
 * per-bank-row workspace of the matching stages (30 B per descriptor of the map and 32 MB), so a rank can afford one per
 * query of a gang.  lender: NULL = a stream of its own, else as sfmloc_context_create_sharing.  Every other asynchronous
 * call on it fails with SFMLOC_EINVAL. */
int sfmloc_context_create_merge(sfmloc_map *map, sfmloc_context *lender, sfmloc_context **out);
int sfmloc_gang_end(sfmloc_context *const *ctxs, uint32_t n);
int sfmloc_gang_counters(sfmloc_context *lead_ctx, uint64_t *launches, uint64_t *gang_launches);
/* Sharded BoW shortlist (selectViewByBoF over a map split by view).  _shard_bow_keys ranks this shard's
 * views against the query's BoW vector (query_bow, or NULL for the resident one) and writes its knn best to keys_dev
 * [knn] as sortable 64-bit keys (float32 distance bits << 32 | view id; ~0 = padding).  The caller all-gathers the key
 * lists; _shard_begin_bow takes the n_parts lists (list p at keys_dev + p*part_stride_keys keys; 0 = back to back),
 * keeps the shard's part of the GLOBAL knn best (ties to the lower view id, as the unsharded sfmloc_bow_select) and
 * runs sfmloc_shard_begin on it -- all on the device, asynchronously.  knn <= 1024, n_parts*knn <= 8192. */
int sfmloc_shard_bow_keys(sfmloc_context *ctx, sfmloc_query *q, const float *query_bow, uint32_t knn, void *keys_dev);
int sfmloc_shard_begin_bow(sfmloc_context *ctx, sfmloc_query *q, const void *keys_dev, uint32_t n_parts,
                           uint64_t part_stride_keys, uint32_t knn);
/* part p starts at parts_dev + p*part_stride (part_stride = 0 means sfmloc_part_bytes(cap): back to back) */
int sfmloc_merge_begin(sfmloc_context *ctx, sfmloc_query *q, const void *parts_dev, uint32_t n_parts, uint32_t cap,
                       uint64_t part_stride);
/* ... then sfmloc_localize_end(ctx, ...) */
/* The exchange of a whole BATCH in one buffer per shard ("packed part"): header {u32 total, n_queries, budget, flags},
 * u32 count[n_queries], u32 offset[n_queries], then (16-byte aligned) the candidates of all the batch's queries back
 * to back -- a shard sends what it found (a few MB per 256-query batch) instead of n_queries fixed-capacity parts.
 *   sfmloc_packed_bytes(n_queries, budget)   size of one packed part holding up to `budget` candidates in all;
 *   sfmloc_shard_export_packed               appends the context's candidates (after sfmloc_shard_begin[_bow]) as query
 *                                            `query_index` of the batch; the caller zeroes the first 16 bytes of
 *                                            packed_dev before the batch's first export.  When the budget does not
 *                                            suffice the query is recorded empty, flags |= 1, and `total` still counts
 *                                            every candidate: after the all-gather every rank sees total > budget and
 *                                            repeats the batch with a larger budget;
 *   sfmloc_merge_begin_packed                sfmloc_merge_begin over the gathered packed parts (part p at packed_dev +
 *                                            p*part_stride; 0 = back to back) for the batch's query `query_index`. */
uint64_t sfmloc_packed_bytes(uint32_t n_queries, uint32_t budget);
int sfmloc_shard_export_packed(sfmloc_context *ctx, void *packed_dev, uint32_t n_queries, uint32_t budget,
                               uint32_t query_index);
int sfmloc_merge_begin_packed(sfmloc_context *ctx, sfmloc_query *q, const void *packed_dev, uint32_t n_parts,
                              uint64_t part_stride, uint32_t n_queries, uint32_t budget, uint32_t query_index);
/* A rank's whole batch per call: the per-query calls above for n_queries queries, in gang sessions of
 * `gang` contexts (query i on context i mod n_ctx; the contexts [g, g + gang) of every n_ctx consecutive queries form one
 * session) -- what a caller would otherwise issue as one foreign call per query and stage.  Asynchronous like the calls
 * they stand for; same results.
 *   _bow_keys      keys_dev [n_queries][knn] u64: every query's knn best views of this shard (resident BoW vectors)
 *   _begin_bow     keys_all_dev [n_parts][n_queries][knn]: the all-gathered keys; stage 1 of every query on its part of
 *                  the global shortlist + its candidates exported to packed_dev (sfmloc_packed_bytes(n_queries, budget))
 *   _begin         the same without a shortlist (every view of the shard)
 *   sfmloc_merge_batch_begin   stage 2 (2D-3D set + P3P) of n <= 32 queries in one session: context k takes query
 *                  query_index[k] of the batch, whose parts lie in packed_all_dev (n_parts parts, part_stride bytes
 *                  apart); finish each with sfmloc_localize_end */
int sfmloc_shard_batch_bow_keys(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                                uint32_t n_queries, uint32_t knn, void *keys_dev);
int sfmloc_shard_batch_begin_bow(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                                 uint32_t n_queries, const void *keys_all_dev, uint32_t n_parts, uint32_t knn,
                                 void *packed_dev, uint32_t budget);
int sfmloc_shard_batch_begin(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                             uint32_t n_queries, void *packed_dev, uint32_t budget);
int sfmloc_merge_batch_begin(sfmloc_context *const *ctxs, uint32_t n, sfmloc_query *const *queries,
                             const uint32_t *query_index, const void *packed_all_dev, uint32_t n_parts,
                             uint64_t part_stride, uint32_t n_queries, uint32_t budget);

/* ------------------------------------------------------------------------- */
/* Stage A5: bag-of-words view shortlist.                                        */
/* sfmloc_bow_select replaces hulo::selectViewByBoF (BoFUtils.cpp:27-68) with the */
/* exact k-NN its FLANN KD-tree approximates: the k candidate views whose .bow    */
/* vector (as float32, BoFUtils.cpp:43-45) is nearest in L2 to the query's; ties  */
/* to the lower view; result ascending (the reference returns a std::set).        */
/* cand_views: ascending view-table indices or NULL for all; requires k < n_cand  */
/* (CV_Assert, BoFUtils.cpp:30); callers skip the shortlist when the candidate    */
/* set is not larger than k (localization.cpp:346).  Synchronises.                */
/* ------------------------------------------------------------------------- */
int sfmloc_bow_select(sfmloc_map *map, const float *query_bow, const uint32_t *cand_views, uint32_t n_cand,
                      uint32_t k, uint32_t *out_sel, uint32_t *n_out);
/* The distances sfmloc_bow_select ranks by: out_dist[v] = the float32 L2 distance of view v's .bow vector to the
 * query's (same kernel, same summation order).  For the sharded shortlist: every rank ranks its own
 * views, the ranks exchange their k best (distance, view id) pairs and keep the global k best; ties go to the lower
 * view id, as in the unsharded selection. */
int sfmloc_bow_distances(sfmloc_map *map, const float *query_bow, float *out_dist /*[n_views]*/);

/* The query's BoW vector from its dense local features: PcaWrapper::calcPcaProject (PcaWrapper.cpp:67-89) +
 * BoFSpatialPyramids::calcBoF (BoFSpatialPyramids.cpp:108-302) with an exact nearest-centre search.
 * Model = what BOWfile.yml / PCAfile.yml hold (BoFSpatialPyramids.cpp:57-83, PcaWrapper.cpp:53-65). */
typedef struct sfmloc_bof_desc {
  int K;                     /* "K" */
  int in_dim;                /* dense descriptor length (61 for M-LDB bytes as floats) */
  const float *centers;      /* "Centers" [K x (n_pca ? n_pca : in_dim)] */
  int resized_image_size;    /* "ResizedImageSize" (300) */
  int use_spatial_pyramid;   /* "UseSpatialPyramid" */
  int pyramid_level;         /* "PyramidLevel" (2) */
  int norm_type;             /* "NormBofFeatureType": 0 NONE, 1 L2, 2 L1 (square root) */
  int n_pca;                 /* "DimPCA", 0 = no PCA */
  const float *pca_mean;     /* "MeanPCA" [in_dim] */
  const float *pca_eigvec;   /* "EigenVectorsPCA" first n_pca rows [n_pca x in_dim] */
  const float *pca_eigval;   /* "EigenValuesPCA" first n_pca */
} sfmloc_bof_desc;
typedef struct sfmloc_bof sfmloc_bof;
int sfmloc_bof_create(const sfmloc_bof_desc *desc, int device, sfmloc_bof **out);
void sfmloc_bof_destroy(sfmloc_bof *bof);
int sfmloc_bof_dim(const sfmloc_bof *bof); /* K x pyramid cells (500) */
/* desc [n x in_dim] f32, kpt_xy [n x 2] in the resized image; out_bow [sfmloc_bof_dim] f64.  Synchronises. */
int sfmloc_bof_compute(sfmloc_bof *bof, const float *desc, const float *kpt_xy, uint32_t n, double *out_bow);

/* ------------------------------------------------------------------------- */
/* Stage A2 / A5a: AKAZE detection and full 486-bit M-LDB description.            */
/* sfmloc_akaze_detect_and_compute replaces                                        */
/*   cv::AKAZE::create(DESCRIPTOR_MLDB, 0, 3, thres, nOct, nOctLay)->detectAndCompute(gray, noArray(), kpts, desc) */
/* (AKAZEOpenCV.cpp:44-46,67); sfmloc_akaze_compute replaces extractor->compute(gray, keypoints, desc) on given  */
/* keypoints (DenseLocalFeatureWrapper.cpp:146; class_id = evolution level, octave 0).                           */
/* An extractor is bound to one image size (it owns the scale-space buffers).                                    */
/*   limits (sfmloc_akaze_create, SFMLOC_EINVAL beyond): width 16 .. 16384, height 16 .. 4096; n_octaves 1 .. 8,    */
/*   n_sublevels >= 1, n_octaves * n_sublevels <= 32; and no evolution level may need more than 64 diffusion (FED)  */
/*   steps -- the steps of a level depend on its octave and sub-level alone: octaves 0 .. 4 never do (63 at most),  */
/*   an octave 5 that survives the cut (a frame of 2560 x 1280 or more with n_octaves >= 6) does; the text names    */
/*   the level and its step count.  More than 65 536 extrema candidates in one image: SFMLOC_ECAP from the call.    */
/*   kpts [cap*6]: x, y, size (diameter), angle (radians), response, class_id                                    */
/*   desc64 [cap*64]: rows exactly as saveAKAZEBin stores them (61 M-LDB bytes + 3 zero bytes, FileUtils.cpp:77-92) */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_akaze sfmloc_akaze;
int sfmloc_akaze_create(int device, int width, int height, int n_octaves, int n_sublevels, float threshold,
                        sfmloc_akaze **out);
void sfmloc_akaze_destroy(sfmloc_akaze *ak);
int sfmloc_akaze_detect_and_compute(sfmloc_akaze *ak, const uint8_t *gray, float *kpts, uint8_t *desc64, uint32_t cap,
                                    uint32_t *n_out);
/* n images of ONE size at once, extractor i taking image i (1 <= n <= 32): the scale spaces, determinants and extrema of
 * all of them go out as one launch per kernel (a gang session on the first extractor's stream) -- these are launch-bound
 * kernels on small images, eight frames cost little more than one --, the candidates' refinement on the host and the
 * orientation + M-LDB launch follow per image.  kpts[i] / descs[i] / n_out[i] as in the single call; same results. */
int sfmloc_akaze_detect_and_compute_batch(sfmloc_akaze *const *aks, const uint8_t *const *grays, uint32_t n,
                                          float *const *kpts, uint8_t *const *descs, uint32_t cap, uint32_t *n_out);
/* kin [n*4]: x, y, size, class_id */
/* detectAndCompute whose outputs stay on the device, laid out as a query block (what extractAKAZESingleImg hands
 * matchAKAZEToQuery, AKAZEOpenCV.cpp:37-113, without the .feat / .desc files in between): descriptor rows [n x 64]
 * followed by zero rows up to a multiple of 64, keypoints (x, y) float2 [n], the keypoints after the .feat text round
 * trip (6 significant digits, AKAZEOpenCV.cpp:80-81,106-111) float2 [n], and the six-float records [n x 6].  Only the
 * counts come back: ONE host synchronisation per call, nothing else crosses PCIe.  _resident_arrays: the device addresses
 * (valid until the extractor's next call) -- sfmloc_query_create_view(map, desc, kpt, kpt6, bow, n, w, h) makes the query;
 * queue its localisation on the extractor's stream (sfmloc_akaze_share_stream) or synchronise in between. */
int sfmloc_akaze_detect_resident(sfmloc_akaze *ak, const uint8_t *gray, uint32_t *n_out);
int sfmloc_akaze_detect_resident_batch(sfmloc_akaze *const *aks, const uint8_t *const *grays, uint32_t n, uint32_t *n_out);
int sfmloc_akaze_resident_arrays(sfmloc_akaze *ak, const void **desc_dev, const void **kpt_dev, const void **kpt6_dev,
                                 const void **kp6_dev);
int sfmloc_akaze_compute(sfmloc_akaze *ak, const uint8_t *gray, const float *kin, uint32_t n, uint8_t *desc64,
                         float *angle_out);
/* scale-space introspection for parity tests: level sizes, and the stacked Ldet / Lt images of the last call */
int sfmloc_akaze_levels(const sfmloc_akaze *ak, int *n_levels, int *wh);
/* From now on the extractor queues its work on the context's stream (ctx = NULL: back on its own).  A server worker that
 * extracts an image and then localises it with that context (localizeImage.cc:149-177 then LocalizeEngine::localize) does
 * the two one after the other anyway; with one stream it occupies one hardware queue instead of two, and concurrent
 * workers stop competing for queues (profiles/r02_image_in_sweep.txt).  The context must outlive the sharing. */
int sfmloc_akaze_share_stream(sfmloc_akaze *ak, sfmloc_context *ctx);
int sfmloc_akaze_read_levels(sfmloc_akaze *ak, float *ldet, float *lt);
/* the duplicate suppression of the last call from the inside (kpts_aux of AKAZEFeatures.cpp, Find_Scale_Space_Extrema): out9 =
 * extrema candidates, keypoints, rounds of the first pass, three in-kernel clocks (10 ns ticks: first pass, second pass,
 * compaction), candidates whose A / P neighbour lists spilled (decided by band scans), whose N list spilled, levels decided
 * out of the global arrays instead of LDS.  SFMLOC_AKAZE_SUPPRESS=spill / global (read by sfmloc_akaze_create) forces
 * those forms; results are the same bits. */
int sfmloc_akaze_suppress_stats(sfmloc_akaze *ak, uint32_t *out9);

/* cv::imread of the query image, host side (AKAZEOpenCV.cpp:60 `imread(filename, IMREAD_GRAYSCALE)` for extraction;
 * DenseLocalFeatureWrapper.cpp:85 and localizeImage.cc:463 `IMREAD_COLOR` for the dense-BoW front end).  Decodes
 * JPEG (baseline / extended / progressive Huffman, 8 bit, 4:4:4 / 4:2:2 / 4:2:0 / gray -- libjpeg's default path
 * restated: islow IDCT, fancy upsampling, fixed-point YCbCr->RGB; gray = the Y plane as JCS_GRAYSCALE gives it), PNG
 * (8 bit, non-interlaced; colour -> gray as png_set_rgb_to_gray(1, .299, .587)) and binary PGM / PPM.
 * color == 0: out is h x w gray; color != 0: out is h x w x 3 in B G R order.  With out == NULL only *width and
 * *height are returned (size query).  SFMLOC_EIO for a file that cannot be read or decoded, SFMLOC_ECAP when `cap`
 * bytes do not hold the image.  No device is needed. */
int sfmloc_image_decode(const uint8_t *bytes, uint64_t n_bytes, int32_t color, uint8_t *out, uint64_t cap,
                        int32_t *width, int32_t *height);
int sfmloc_image_read(const char *path, int32_t color, uint8_t *out, uint64_t cap, int32_t *width, int32_t *height);

/* cv::imread whose pixels are born on the device.  A JPEG's header parsing and entropy stage (Huffman: serial) run on
 * the host exactly as in sfmloc_image_decode, once per file; the coefficient blocks cross PCIe in one upload and two
 * kernels reconstruct (dequantisation + islow IDCT; fancy upsampling + colour).  Up to three images stay resident,
 * chosen by the mask `want`; every pixel equals what sfmloc_image_decode returns for the same bytes:
 *   SFMLOC_IMREAD_GRAY      h x w       imread(IMREAD_GRAYSCALE)
 *   SFMLOC_IMREAD_BGR       h x w x 3   imread(IMREAD_COLOR)
 *   SFMLOC_IMREAD_BGR2GRAY  h x w       cvtColor(imread(IMREAD_COLOR), COLOR_BGR2GRAY) (localizeImage.cc:463)
 * PNG and binary PGM / PPM files are decoded on the host as sfmloc_image_decode does and uploaded, so that a consumer
 * has one route for every format.  _create: frames of at most max_width x max_height (each 1 .. 16384); everything is
 * allocated here, a JPEG call allocates nothing.  _decode / _file: all parsing happens before anything is queued -- a
 * file sfmloc_image_decode refuses gives its code and its text after "sfmloc_imread_decode: ", nothing is launched and
 * the previous images stand; a frame larger than the reader's maximum is SFMLOC_ECAP.  The calls queue their work on
 * the reader's stream and return: the one host wait is for the PREVIOUS call's upload to have left the pinned staging
 * buffer.  _read waits and copies one image out (parity tests, host consumers); _dev is its device address (NULL when
 * the last decode did not leave it), valid until the next decode; its contents are ordered on the reader's stream --
 * the consumers below order themselves behind it with an event.  _share_stream: as sfmloc_akaze_share_stream.
 * _timing: enable != 0 makes the following JPEG decodes record events; out4 (may be NULL) = the last timed decode's
 * host milliseconds (header + entropy stage + staging) and device milliseconds of the upload, the IDCT launch and the
 * upsampling / colour launch, after waiting for them. */
#define SFMLOC_IMREAD_GRAY 1
#define SFMLOC_IMREAD_BGR 2
#define SFMLOC_IMREAD_BGR2GRAY 4
typedef struct sfmloc_imread sfmloc_imread;
int sfmloc_imread_create(int device, uint32_t max_width, uint32_t max_height, sfmloc_imread **out);
void sfmloc_imread_destroy(sfmloc_imread *r);
int sfmloc_imread_decode(sfmloc_imread *r, const uint8_t *bytes, uint64_t n_bytes, uint32_t want, int32_t *width,
                         int32_t *height);
int sfmloc_imread_file(sfmloc_imread *r, const char *path, uint32_t want, int32_t *width, int32_t *height);
int sfmloc_imread_read(sfmloc_imread *r, uint32_t which, uint8_t *out, uint64_t cap);
const void *sfmloc_imread_dev(const sfmloc_imread *r, uint32_t which);
int sfmloc_imread_share_stream(sfmloc_imread *r, sfmloc_context *ctx);
int sfmloc_imread_timing(sfmloc_imread *r, int32_t enable, double *out4);
/* The extractors on a reader's resident image instead of a host pointer: `which` names ONE image of the reader's last
 * decode (a gray one), whose size must be the extractor's (SFMLOC_EINVAL otherwise).  The extractor's stream is ordered
 * behind the reader's work with an event, not a host wait; otherwise as sfmloc_akaze_detect_resident /
 * sfmloc_akaze_detect_and_compute: one host synchronisation per frame, for the keypoint count. */
int sfmloc_akaze_detect_resident_dev(sfmloc_akaze *ak, sfmloc_imread *r, uint32_t which, uint32_t *n_out);
int sfmloc_akaze_detect_and_compute_dev(sfmloc_akaze *ak, sfmloc_imread *r, uint32_t which, float *kpts, uint8_t *desc64,
                                        uint32_t cap, uint32_t *n_out);

/* The server's per-user image undistortion in front of LocalizeEngine::localize (localizeImage.cc:149-177, SURVEY
 * 8f-4).  _create = the once-per-camera part, host arithmetic only (no device needed):
 *   newCameraMat = getOptimalNewCameraMatrix(K, dist, size, 1.0, size, &validRoi)  +  cv::undistort's CV_16SC2 maps;
 * _apply = the per-image part on the GPU: undistort(image, K, dist, newCameraMat) then the crop to validRoi --
 * fixed-point bilinear remap, zero border.  K row-major 3x3; dist = k1 k2 p1 p2 [k3 [k4 k5 k6]] (n_dist 0, 4, 5, 8).
 * src: height x width x channels (1 or 3) u8; dst: roi_h x roi_w x channels.  _info: new camera matrix [9] and
 * validRoi [4] = x y w h; _maps: the full-size maps (xy [h*w*2] i16, frac [h*w] u16 = fy<<5|fx) for parity tests. */
typedef struct sfmloc_undistorter sfmloc_undistorter;
int sfmloc_undistorter_create(int device, const double *K, const double *dist, uint32_t n_dist, uint32_t width,
                              uint32_t height, sfmloc_undistorter **out);
void sfmloc_undistorter_destroy(sfmloc_undistorter *u);
int sfmloc_undistorter_info(const sfmloc_undistorter *u, double *new_camera, int32_t *roi);
int sfmloc_undistorter_maps(const sfmloc_undistorter *u, int16_t *xy, uint16_t *frac);
int sfmloc_undistorter_apply(sfmloc_undistorter *u, const uint8_t *src, uint32_t channels, uint8_t *dst, uint64_t cap);

/* Dense-BoW front end (DenseLocalFeatureWrapper.cpp:89-99): colour image (BGR, 8-bit,
 * row-major h x w x 3) -> cv::resize(size x size, INTER_CUBIC) -> BGR2GRAY -> normalize(0, 255, NORM_MINMAX);
 * gray_out [size*size].  The grid keypoints (DenseFeatureDetector.cpp:44-69) and the chaining into
 * sfmloc_akaze_compute / sfmloc_bof_compute are host glue (sfmlocalization_amd/engine.py::dense_bow). */
int sfmloc_dense_gray(int device, const uint8_t *bgr, uint32_t width, uint32_t height, uint32_t size,
                      uint8_t *gray_out);

/* The query-side BoW vector from the IMAGE as one resident, asynchronous chain: replaces, per
 * query, DenseLocalFeatureWrapper::calcDenseLocalFeature (BoWCommon/src/DenseLocalFeatureWrapper.cpp:83-183) ->
 * PcaWrapper::calcPcaProject (VisionLocalizeCommon/src/PcaWrapper.cpp:67-89) -> BoFSpatialPyramids::calcBoF
 * (BoWCommon/src/BoFSpatialPyramids.cpp:108-302) as localization.cpp:346-361 / LocalizeEngine.cc:205-232 call them.
 * _create: everything an image of this size needs is allocated once (model = the BOWfile.yml / PCAfile.yml contents as
 * for sfmloc_bof_create; in_dim must be 61; channels 3 = BGR as imread(IMREAD_COLOR) returns it, 1 = a gray image,
 * whose colour read has three equal channels).  _compute: image [height x width x channels] in host memory -> the
 * vector; nothing is allocated, nothing crosses PCIe but the image (and the result when out_bow is given).
 *   query   non-NULL: the float32 vector (what BoFUtils.cpp:51-54 hands the matcher) is written into the query's
 *           resident BoW slot, as sfmloc_query_set_bow would, ASYNCHRONOUSLY on the extractor's stream: share that
 *           stream with the context that will localise the query (sfmloc_imgbow_share_stream) so that
 *           sfmloc_localize_bow_begin(ctx, query, NULL, knn) is ordered after it, or pass out_bow (which synchronises).
 *   out_bow non-NULL: the reference's float64 vector [sfmloc_imgbow_dim], after a stream synchronisation.
 * Same kernels as sfmloc_dense_gray + sfmloc_akaze_compute + sfmloc_bof_compute: the same bits. */
typedef struct sfmloc_imgbow sfmloc_imgbow;
int sfmloc_imgbow_create(const sfmloc_bof_desc *model, int device, uint32_t width, uint32_t height, uint32_t channels,
                         sfmloc_imgbow **out);
void sfmloc_imgbow_destroy(sfmloc_imgbow *ib);
int sfmloc_imgbow_dim(const sfmloc_imgbow *ib);
int sfmloc_imgbow_share_stream(sfmloc_imgbow *ib, sfmloc_context *ctx); /* NULL: back on its own stream */
int sfmloc_imgbow_compute(sfmloc_imgbow *ib, const uint8_t *image, sfmloc_query *query, double *out_bow);
/* the same from a reader's resident image (sfmloc_imread_decode): `which` = SFMLOC_IMREAD_BGR for a 3-channel
 * extractor, a gray image for a 1-channel one; the frame's size must be the extractor's (SFMLOC_EINVAL otherwise).
 * Nothing crosses PCIe; the extractor's stream waits for the reader's work through an event. */
int sfmloc_imgbow_compute_dev(sfmloc_imgbow *ib, sfmloc_imread *r, uint32_t which, sfmloc_query *query, double *out_bow);
/* The vectors of n frames (1..32) in ONE gang session on the first extractor's stream: one launch per kernel for all of
 * them; the float32 vectors stay on the device (sfmloc_imgbow_vector_dev of each extractor).  The reference computes the
 * vector per query image (localization.cpp:346-361, LocalizeEngine.cc:205-232); same bits as n single calls. */
int sfmloc_imgbow_compute_batch(sfmloc_imgbow *const *ibs, const uint8_t *const *images, uint32_t n);
/* the reference's float64 vector of the extractor's last call (single or batch), after waiting for it */
int sfmloc_imgbow_vector_read(sfmloc_imgbow *ib, double *out_bow);
/* where the float32 vector of a call WITHOUT a query lands (device memory, [sfmloc_imgbow_dim] floats): the bow_dev of a
 * query view (sfmloc_query_create_view) over an extractor's resident outputs */
const void *sfmloc_imgbow_vector_dev(const sfmloc_imgbow *ib);
/* an extractor on a stream of its own (not shared) works beside the feature extraction of the same frame; this makes the
 * context's stream wait for everything the extractor has queued so far (call it before sfmloc_localize_bow_begin) */
int sfmloc_imgbow_order_before(sfmloc_imgbow *ib, sfmloc_context *ctx);

/* Vocabulary training (TrainBoW/src/TrainBoW.cpp): the device-resident training sample, PCA and k-means behind
 * BOWfile.yml / PCAfile.yml.  All work is queued on the trainer's own non-blocking stream; every reduction runs in a
 * fixed order, so two runs give the same bytes.  Fixed arithmetic (the test restates it):
 *   rows are f32 [n x dim], dim <= 64; "chunk" = 1024 consecutive rows;
 *   moments: Sx, Sxx summed in f64 sequentially within a chunk, chunks added in order (exact for integer rows);
 *     mean = Sx / N, cov = (Sxx - N * (mean_i * mean_j)) / N (cv::PCA, CV_COVAR_SCALE); cyclic Jacobi on the host,
 *     eigenvalues descending, each eigenvector's largest-magnitude component positive (first such on ties);
 *   projection: bof_device.h, the arithmetic of sfmloc_bof_compute's PCA step (project, divide by the eigenvalue);
 *   distance = sum_d (x_d - c_d)^2 in f32, dimension order, unfused; ties to the lower centre index;
 *   k-means++ (generateCentersPP, 3 local trials): first centre next() % N; a trial draws u = (double)rng and takes the
 *     first i whose running sum R_i >= u * total, R_i = (sum of the partials of the chunks before i's) + (sum within
 *     i's chunk up to i), each sum f64 and sequential (N - 1 if none); total = the chunk partials added in order;
 *   Lloyd (cv::kmeans, OpenCV 3 shape): centre sums in f64 (per chunk sequential, chunks in order), divided by the
 *     count in f64, rounded to f32; an empty cluster takes the biggest cluster's (first on ties) farthest point (the
 *     last on ties) from that cluster's centre (f32 of sum / count); squared shift in f64; stop when ++iter ==
 *     max(max_iter, 2) or the largest shift <= eps^2; the min distances and compactness (their f64 chunked sum) are
 *     those of the last assignment, the labels those of the last assignment after the last centre step's empty-cluster
 *     moves (as cv::kmeans returns them); best of `attempts`, the first wins ties.
 *   cv::RNG: state = (u64)(u32)state * 4164903690 + (state >> 32), next() = (u32)state; uniform(0.f, 1.f) =
 *     (float)next() * 2^-32; (double)rng = ((u64)next() << 32 | next()) * 2^-64; state 0 means 0xffffffff. */
typedef struct sfmloc_bowtrain sfmloc_bowtrain;
/* cap_rows: sample capacity; dim: row length (61 for the dense M-LDB rows) */
int sfmloc_bowtrain_create(int device, uint32_t dim, uint32_t cap_rows, sfmloc_bowtrain **out);
void sfmloc_bowtrain_destroy(sfmloc_bowtrain *t);
int sfmloc_bowtrain_reset(sfmloc_bowtrain *t); /* empty the sample (dim back to the created one) */
int sfmloc_bowtrain_add_rows(sfmloc_bowtrain *t, const float *rows, uint32_t n); /* host rows [n x dim] */
/* getRandomTrainFeatures' body for one draw (TrainBoW.cpp:106-125): the image's dense descriptors (the chain of
 * sfmloc_dense_gray + sfmloc_akaze_compute on the 300 x 300 dense grid, 61 bytes as f32), then n_pick rows
 * k = min((int)(rows * uniform(0.f, 1.f)), rows - 1) drawn from *rng_state and gathered on the device.  bgr == NULL:
 * an image without descriptors -- its n_pick rows stay zero and nothing is drawn.  The descriptors of the last image are
 * kept: the same image again (same bytes) is not extracted again (the reference extracts it again: same bits). */
int sfmloc_bowtrain_add_image(sfmloc_bowtrain *t, const uint8_t *bgr, uint32_t w, uint32_t h, uint32_t channels,
                              uint32_t n_pick, uint64_t *rng_state);
int sfmloc_bowtrain_size(const sfmloc_bowtrain *t, uint32_t *n, uint32_t *dim);
int sfmloc_bowtrain_read(sfmloc_bowtrain *t, float *rows, uint64_t cap_floats); /* the sample [n x dim], synchronises */
/* cv::PCA(sample, noArray(), DATA_AS_ROW) (PcaWrapper.cpp:31-46): f64 results (each pointer may be NULL):
 * mean [dim], cov [dim x dim], eigvec [dim x dim] (rows), eigval [dim] */
int sfmloc_bowtrain_pca64(sfmloc_bowtrain *t, double *mean, double *cov, double *eigvec, double *eigval);
/* the same as PCAfile.yml holds it: MeanPCA [1 x dim], EigenVectorsPCA [dim x dim], EigenValuesPCA [dim x 1] f32 */
int sfmloc_bowtrain_pca(sfmloc_bowtrain *t, float *mean, float *eigvec, float *eigval);
/* PcaWrapper::calcPcaProject (TrainBoW.cpp:213): sample -> pca->n_pca columns, in place (pca->in_dim == dim) */
int sfmloc_bowtrain_project(sfmloc_bowtrain *t, const sfmloc_bof_desc *pca);
/* BoFSpatialPyramids::trainKMeans (BoFSpatialPyramids.cpp:95-106): cv::kmeans(sample, min(K, n), labels,
 * TermCriteria(COUNT + EPS, max_iter, eps), attempts, KMEANS_PP_CENTERS), k-means++ draws from cv::RNG(seed).
 * min(K, n) x dim x 8 + min(K, n) x 4 bytes must fit 64 KB (the centre sums' workgroup memory): K <= 132 at dim 61,
 * K <= 248 at dim 32; SFMLOC_EINVAL otherwise.  centers [min(K, n) x dim]; labels [n], min_dist [n] (f32 distance to
 * the assigned centre), compactness, iterations (assignments run, all attempts together): each may be NULL. */
int sfmloc_bowtrain_kmeans(sfmloc_bowtrain *t, uint32_t K, uint32_t attempts, uint32_t max_iter, double eps,
                           uint64_t seed, float *centers, int32_t *labels, float *min_dist, double *compactness,
                           uint32_t *iterations);

/* ------------------------------------------------------------------------- */
/* Re-resection and structure cleanup of a whole sfm_data (OpenMVG_BA/src/adjust_sfm_data.cpp without -c, the call   */
/* the reference's merge loop makes once per candidate merge).  The sfm_data stays resident on the device: view table, */
/* intrinsics, poses, landmark X and the observations in CSR by landmark.  Semantics restated (OpenMVG 1.1 points are */
/* unpinned readings; each says which reading was chosen):                                                             */
/*   views       a view is resected iff it has more than 10 observations (MINIMUM_VIEW_NUM_TO_ESTIMATAE_CAMERA_POSE, */
/*               test ">", :118); the others are left untouched and the tool warns "there is/are frames with too few  */
/*               matches" (:148-150).  Its correspondences are (obs.x, X) in ascending landmark id (std::map order of */
/*               Landmarks, :100-107), built on the device by a stable radix sort of the observations by view.        */
/*   raw pixels  (quirk kept) resection_data.pt2D holds the RAW obs.x (:107-115); the undistorted pt2D of :125-131 is   */
/*               never used, so P3P gets raw pixels and K = (f, ppx, ppy) of the view's intrinsic even for            */
/*               pinhole_radial_k3.                                                                                    */
/*   resection   K5 (SfM_Localizer::Localize: P3P AC-RANSAC, params.p3p_max_iteration = 4096, error_max infinite) with */
/*               its own gate vec_inliers > 2.5 * 3, i.e. >= 8 inliers (params.min_inliers = 7; the localiser's       */
/*               MINUM_NUMBER_OF_INLIER_RESECTION does not apply; params.min_resection_points = 10: the view rule).   */
/*               The sampling stream is the view's id_view, so a view's result does not depend on the batch.          */
/*   success     pose[id_pose] = Pose3(R, -R^T t) of KRt_From_P(P) (:138-142), inserted if the pose id had none.      */
/*               Views sharing a pose id: the last view in ascending id wins (the reference races, :91).              */
/*   limit       (divergence) a view with more than 65 536 observations is refused (SFMLOC_ECAP): its list must fit  */
/*               a K5 context's 2D-3D buffers.  The reference has no such limit.                                      */
/*   failure     (divergence) the reference stores a pose built from an uninitialised Mat34 (Localize never sets the */
/*               projection matrix on failure); here the view keeps its input pose, or stays without one.             */
/*   residual    RemoveOutliers_PixelResidualError(4.0): an observation goes when                                     */
/*               sqrt(dx*dx + dy*dy) > 4.0, (dx, dy) = obs.x - cam2ima(add_disto(hnormalized(R (X - C)))) of its     */
/*               view's pose and intrinsic; a landmark left with fewer than 2 observations goes.  Arithmetic (f64,     */
/*               unfused, in this order): d = X - C; Xc_i = (R_i0 d0 + R_i1 d1) + R_i2 d2; p = (Xc0 / Xc2, Xc1 / Xc2);*/
/*               radial: r2 = p0 p0 + p1 p1, r4 = r2 r2, r6 = r4 r2, p *= ((1 + k1 r2) + k2 r4) + k3 r6;           */
/*               proj = f p + pp.  An observation whose view has no pose is an error (GetPoseOrDie throws).          */
/*   angle       RemoveOutliers_AngleError(2.0): a landmark goes when the largest angle over all pairs of its        */
/*               remaining observations is < 2 degrees.  Reading chosen: the bearing undistorts first (get_ud_pixel, */
/*               the bisection of geom_device.h), b = (u, v, 1) with (u, v) = ((x - ppx) / f, (y - ppy) / f),         */
/*               normalised by sqrt((u u + v v) + 1); ray = R^T b (ray_i = (R_0i b0 + R_1i b1) + R_2i b2); per pair */
/*               c = dot / (|r1| |r2|) (dot and squared norms summed x, y, z in order), clamped as OpenMVG's         */
/*               clamp does, max(lo, min(c, hi)) with lo = -1 + 1e-8, hi = 1 - 1e-8 (a NaN cosine becomes lo: 180    */
/*               degrees, the track stays); the landmark keeps the minimum c and goes when acos(c) * 180 / pi < 2.    */
/*               (A NaN residual norm is not > 4.0: the observation stays.)                                          */
/*   unstable    (-r=1) eraseUnstablePosesAndObservations(6, 2): erase every pose with fewer than 6 observations     */
/*               (counted per id_pose; a pose nobody observes has 0), then every observation whose view's pose is    */
/*               gone and every landmark left with fewer than 2; repeat while observations were removed.            */
/* No float atomics and no order-dependent atomics: two runs give the same bits.                                        */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_sfm_desc {
  uint32_t n_views;
  const uint32_t *view_id;         /* [n_views] id_view, strictly ascending (Views is a std::map) */
  const uint32_t *view_intrinsic;  /* [n_views] index into the intrinsic table */
  const uint32_t *view_pose;       /* [n_views] index into the pose table (the view's id_pose) */
  uint32_t n_intrinsics;
  const uint32_t *intrinsic_type;  /* [n_intrinsics] 0 pinhole, 3 pinhole_radial_k3; any other: SFMLOC_EIO */
  const double *intrinsic;         /* [n_intrinsics*6] focal, ppx, ppy, k1, k2, k3 (zeros for pinhole) */
  uint32_t n_poses;                /* the pose table: every extrinsic key and every view's id_pose, ascending id */
  const uint8_t *pose_valid;       /* [n_poses] 1 = the input has this extrinsic */
  const double *pose_R;            /* [n_poses*9] rotation, row major */
  const double *pose_C;            /* [n_poses*3] centre */
  uint32_t n_landmarks;
  const uint32_t *landmark_id;     /* [n_landmarks] strictly ascending (Landmarks is a std::map) */
  const double *landmark_X;        /* [n_landmarks*3] */
  const uint64_t *obs_off;         /* [n_landmarks+1] CSR by landmark, obs_off[0] = 0 */
  const uint32_t *obs_view;        /* [n_obs] view index (into the view table) */
  const double *obs_x;             /* [n_obs*2] pixel */
} sfmloc_sfm_desc;

typedef struct sfmloc_sfm_view_result {
  int32_t ran;         /* 1 = resected (more than 10 observations) */
  int32_t ok;          /* 1 = Localize succeeded (>= 8 inliers): the view's pose was replaced */
  int32_t n_obs;       /* correspondences of the view */
  int32_t n_inliers;   /* AC-RANSAC's inlier count, success or not (0 when no model has a negative NFA) */
  int32_t iterations;  /* AC-RANSAC iterations run */
  int32_t reserved;
  double error_max, nfa;
  double P[12];        /* K [R|t] of AC-RANSAC's best model, success or not (zeros without inliers) */
  double R[9], center[3];  /* KRt_From_P(P), R and -R^T t: only when ok (zeros otherwise; the reference would store
                              a pose of an uninitialised matrix, see "failure") */
} sfmloc_sfm_view_result;

typedef struct sfmloc_sfm sfmloc_sfm;
/* params of the tool: sfmloc_default_params + min_resection_points 10, min_inliers 7, p3p_max_iteration 4096 */
void sfmloc_sfm_default_params(sfmloc_params *p);
int sfmloc_sfm_create(const sfmloc_sfm_desc *desc, const sfmloc_params *params, sfmloc_sfm **out);
void sfmloc_sfm_destroy(sfmloc_sfm *h);
/* re-resects every view with more than 10 observations (gang sessions of 32 contexts); n_ran / n_ok may be NULL */
int sfmloc_sfm_resect(sfmloc_sfm *h, uint32_t *n_ran, uint32_t *n_ok);
int sfmloc_sfm_resect_read(const sfmloc_sfm *h, sfmloc_sfm_view_result *out /*[n_views]*/);
/* the inliers of view k as indices into its correspondence list (ascending landmark id), AC-RANSAC order: for every
 * view that ran, a failed one included (its best model's n_inliers inliers); empty for a view that did not run */
int sfmloc_sfm_resect_inliers(const sfmloc_sfm *h, uint32_t k, uint32_t *idx, uint32_t cap, uint32_t *n);
/* residual + angle filters (+ the unstable-pose loop when rm_unstable); counts = landmarks before, after the residual
 * filter, after the angle filter, after cleanup.  SFMLOC_EINVAL (text names the view) when an observation's view has
 * no pose. */
int sfmloc_sfm_clean(sfmloc_sfm *h, double residual_px, double angle_deg, int rm_unstable, uint64_t *counts /*[4]*/);
/* poses [n_poses] (valid, R, C) and keep masks [n_obs] / [n_landmarks]; any pointer may be NULL */
int sfmloc_sfm_read(sfmloc_sfm *h, uint8_t *pose_valid, double *pose_R, double *pose_C, uint8_t *obs_keep,
                    uint8_t *landmark_keep);
/* debug: residual norm per observation (NaN where not evaluated), minimum clamped cosine per landmark (NaN where the
 * angle filter did not look at it) */
int sfmloc_sfm_debug_read(sfmloc_sfm *h, double *residual, double *min_cos);
/* host only: parse a JSON file and write it back as Python's json.dump does (the tool's writer) */
int sfmloc_sfm_json_rewrite(const char *in_path, const char *out_path);

/* ------------------------------------------------------------------------- */
/* The separable commands of OpenMVG_BA -c (adjust_sfm_data.cpp:158-244): structure alone (s), or the poses alone      */
/* (r, t, rt), on the resident sfm_data.  With the other side and the intrinsics fixed every landmark (3 parameters)   */
/* or every pose (3 or 6) is a problem of its own with a unique minimum; the joint commands (structure with a pose      */
/* part, anything with intrinsics) are refused.  Semantics restated from OpenMVG 1.1's Bundle_Adjustment_Ceres::Adjust  */
/* (all unpinned readings; each says which reading was chosen):                                                         */
/*   blocks      reading chosen, unpinned: a pose is [angle-axis of R (3), t (3)] with t = -R C, t_i =                  */
/*               -((R_i0 C0 + R_i1 C1) + R_i2 C2).  r holds t constant (not C: the centre moves), t holds the rotation  */
/*               constant (its R keeps its bits).  Views that share an id_pose share one block.  After the call        */
/*               C = -R^T t, C_i = -((R_0i t0 + R_1i t1) + R_2i t2).                                                   */
/*   residual    reading chosen, unpinned: two values per observation, proj - obs.x, with the arithmetic of the        */
/*               cleaning residual ("residual" above) on Xc_i = ((R_i0 X0 + R_i1 X1) + R_i2 X2) + t_i: p = (Xc0 / Xc2, */
/*               Xc1 / Xc2), the radial factor ((1 + k1 r2) + k2 r4) + k3 r6 for pinhole_radial_k3, proj = f p + pp.    */
/*               The intrinsics are constants.                                                                          */
/*   loss        reading chosen, unpinned: Ceres HuberLoss(a), a = Square(4.0) = 16 (the squared 4.0 is the reference's */
/*               quirk, kept), on s = |r|^2: rho(s) = s for s <= a^2, else 2 a sqrt(s) - a^2.  cost = 1/2 sum rho.       */
/*   entering    reading chosen, unpinned: the kept observations of kept landmarks (all of them before the first        */
/*               sfmloc_sfm_clean).  One whose view has no pose: SFMLOC_EINVAL, the text names the view.  A pose or a   */
/*               landmark no entering observation refers to keeps its bits.                                             */
/*   solver      reading chosen, unpinned: Levenberg-Marquardt on each block's normal equations (A + lambda D) d = -g,  */
/*               D = diag(A) clamped to [1e-6, 1e32], lambda = 1e-4 at the start; a step is accepted when (cost -       */
/*               cost') / (model decrease) > 1e-3, then lambda *= max(1/3, 1 - (2 q - 1)^3); a rejected step multiplies */
/*               lambda by 2, 4, 8, ...; at most 500 steps tried per block.  The loss enters as the first-order        */
/*               reweighting: residual and Jacobian rows times sqrt(rho'), no second-order (Triggs) correction.  A     */
/*               rotation steps in the tangent space at the current R, R <- exp([w]x) R (divergence: Ceres steps in    */
/*               the angle-axis itself; the path differs, the minimum does not).                                       */
/*   stopping    (divergence) Ceres runs one joint LM with one trust region and stops on the total cost               */
/*               (function_tolerance 1e-6).  Here every block stops on its own: after an accepted step whose relative   */
/*               cost decrease is <= 1e-14, or a rejected one whose model decrease is <= 1e-14 of the cost (the f64     */
/*               floor: below it the cost's own rounding decides), so every block is at least as converged as Ceres     */
/*               leaves it.  A step that does not lower the block's cost is never applied (no block ends above its     */
/*               input cost); a non-finite step or cost counts as rejected.                                           */
/*   order       sums run lane-strided and then through a fixed in-wave butterfly; no float atomics: two runs give    */
/*               the same bits.  The report's totals are summed on the host in ascending block index.                  */
/* ------------------------------------------------------------------------- */
#define SFMLOC_BA_ROTATION 1u
#define SFMLOC_BA_TRANSLATION 2u
#define SFMLOC_BA_INTRINSICS 4u
#define SFMLOC_BA_STRUCTURE 8u
typedef struct sfmloc_ba_report {
  double cost_initial, cost_final; /* 1/2 sum rho over the entering observations, before and after */
  uint32_t n_blocks;               /* blocks with at least one entering observation */
  uint32_t n_at_cap;               /* blocks that tried 500 steps without meeting the stopping rule */
  uint32_t n_unchanged;            /* blocks left at their input (no accepted step) */
  uint32_t max_iterations;         /* the largest number of steps one block tried */
} sfmloc_ba_report;
/* what: 0 (nothing), ROTATION, TRANSLATION, ROTATION | TRANSLATION or STRUCTURE; any other value: SFMLOC_EINVAL, the
 * handle untouched.  rep may be NULL.  A bounded number of launches, no host round trip per iteration.
 * sfmloc_sfm_clean may follow an adjust (and the next adjust a clean): a later clean works on what the earlier one
 * kept, as the reference's second cleanup works on the reduced structure (counts[0] = the landmarks kept so far). */
int sfmloc_sfm_adjust(sfmloc_sfm *h, uint32_t what, sfmloc_ba_report *rep);
/* the landmarks' X as they are now; sfmloc_sfm_read gives the poses */
int sfmloc_sfm_read_structure(sfmloc_sfm *h, double *X /*[n_landmarks*3]*/);

/* ------------------------------------------------------------------------- */
/* The joint commands of OpenMVG_BA -c (rs, rst, rsti, anything with i; adjust_sfm_data.cpp:158-244): poses,           */
/* intrinsics and structure in one problem with one trust region, as Bundle_Adjustment_Ceres::Adjust solves it          */
/* (ITERATIVE_SCHUR, SCHUR_JACOBI; adjust_sfm_data.cpp:175-176).  A new entry point: sfmloc_sfm_adjust keeps refusing  */
/* these commands.  The readings "blocks", "residual", "loss", "entering" and "order" of the separable block above     */
/* carry over word for word (the intrinsics are constants only where the command does not name i).  Added readings:    */
/*   parameters  reading chosen, unpinned: a pose contributes 3 free values for r or t and 6 for rt (r holds t, t      */
/*               holds R's bits).  An intrinsic is free under i: {f, ppx, ppy} for pinhole, plus {k1, k2, k3} for       */
/*               pinhole_radial_k3 (OpenMVG's ADJUST_ALL).  A landmark contributes X under s.  Views that share an      */
/*               id_pose share one block; views that share an id_intrinsic share one block.  A pose, an intrinsic or a  */
/*               landmark no entering observation refers to keeps its bits, and so does everything the command does    */
/*               not name.                                                                                              */
/*   solver      reading chosen, unpinned: one Levenberg-Marquardt loop over the whole problem with one lambda; the    */
/*               start value 1e-4, D = diag(J^T J) clamped to [1e-6, 1e32], the acceptance ratio 1e-3 and the lambda   */
/*               update are those of "solver" above; first-order reweighting, no Triggs correction; rotations step as  */
/*               R <- exp([w]x) R (divergence: Ceres steps in the angle-axis).  With s the landmarks are eliminated    */
/*               (C_l = Jx^T Jx + lambda D inverted by Cholesky) and the reduced system over poses and intrinsics is    */
/*               solved by preconditioned conjugate gradients from x = 0, matrix-free through the observations; without */
/*               s the same PCG runs on Jc^T Jc + lambda D.  The preconditioner is block diagonal, one 6 x 6 block per  */
/*               pose and per intrinsic: J^T J + lambda D minus the block's own -(J^T Jx) C_l^-1 (Jx^T J) terms, taken  */
/*               per observation (divergence: SCHUR_JACOBI also has the cross terms of two observations of one          */
/*               landmark inside one block; they are left out, which weakens the preconditioner and leaves the system   */
/*               solved unchanged).  (divergence) PCG stops at |r| <= pcg_tolerance |r0| in the Euclidean norm, after   */
/*               max_pcg iterations, or when p.Ap is not positive; Ceres has its own Q-based test.  The model decrease  */
/*               is computed from the step actually taken, -(g.d) - |J d|^2 / 2, in one pass over the observations.     */
/*               A step that does not lower the total cost is never applied; a non-finite step or cost counts as        */
/*               rejected.  No gauge fixing (neither OpenMVG 1.1 nor the reference fixes one): the damping carries the  */
/*               7-dimensional null space of rst.                                                                       */
/*   stopping    reading chosen, unpinned: stop 0 after an accepted step with (cost - cost') <= function_tolerance *    */
/*               cost, or after a rejected one whose positive model decrease is itself <= function_tolerance * cost;    */
/*               stop 1 after max_steps steps tried; stop 2 when lambda passes 1e32.                                    */
/*   order       per-pose sums go lane-strided through the in-wave butterfly; per-intrinsic sums and the PCG's scalar   */
/*               products are written as partials (per view, per block, per workgroup) and summed by a fixed tree:      */
/*               store, then sum.  No float atomics: two runs give the same bits.                                       */
/*   after       C = -R^T t for the poses that moved.  sfmloc_sfm_clean, sfmloc_sfm_adjust and further joint calls see  */
/*               the adjusted intrinsics: a later clean uses them.  sfmloc_sfm_resect has already run and is            */
/*               unaffected.                                                                                            */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_ba_joint_options {
  uint32_t max_steps;          /* LM steps tried;      default 50  (Ceres max_num_iterations)                */
  uint32_t max_pcg;            /* PCG iterations/step; default 500 (Ceres max_linear_solver_iterations)      */
  double function_tolerance;   /* default 1e-6 (Ceres): stop after an accepted step with
                                  (cost - cost') <= tol * cost                                              */
  double pcg_tolerance;        /* default 0.1 (Ceres eta): stop PCG at |r| <= tol * |r0|                    */
} sfmloc_ba_joint_options;
typedef struct sfmloc_ba_joint_report {
  double cost_initial, cost_final;
  uint32_t n_pose_blocks, n_intrinsic_blocks, n_landmark_blocks;  /* free blocks with an entering observation */
  uint32_t steps_tried, steps_accepted, pcg_total, pcg_max;
  uint32_t stop;               /* 0 tolerance met, 1 max_steps, 2 lambda overflow / no model decrease       */
} sfmloc_ba_joint_report;
void sfmloc_ba_joint_default_options(sfmloc_ba_joint_options *o);
/* what: any non-zero combination of the four SFMLOC_BA_ bits (the separable ones too: solved as one joint problem);
 * any other bit: SFMLOC_EINVAL.  A view of an entering observation without a pose: SFMLOC_EINVAL, the text names the
 * view.  opt NULL = the defaults; rep may be NULL.  One small read-back per LM step and per chunk of 32 PCG iterations;
 * no host round trip per PCG iteration. */
int sfmloc_sfm_adjust_joint(sfmloc_sfm *h, uint32_t what, const sfmloc_ba_joint_options *opt, sfmloc_ba_joint_report *rep);
/* the intrinsics as they are now: f, ppx, ppy, k1, k2, k3 per intrinsic */
int sfmloc_sfm_read_intrinsics(sfmloc_sfm *h, double *K /*[n_intrinsics*6]*/);

/* ------------------------------------------------------------------------- */
/* Structure from known poses (openMVG_main_ComputeStructureFromKnownPoses, and the last stage of                      */
/* openMVG_main_GlobalSfM, reconstructGraph.py:171): feature tracks from the pairwise matches (sfmloc_tracks), then     */
/* every track triangulated from the views' poses on a resident sfmloc_sfm (sfmloc_sfm_triangulate).  OpenMVG's source  */
/* was not at hand: every point below is a reading chosen here, and tests/structure_np.py restates each operation.      */
/* sfmloc_tracks (TracksBuilder::Build + Filter):                                                                       */
/*   nodes       a node is a global feature row, view_off[v] + feature; an edge joins the two nodes of a match.  The    */
/*               pair list has the layout of sfmloc_geometric_pairs (pair k = views (pairs[2k], pairs[2k+1]) owns       */
/*               match_i/j[offsets[k] .. offsets[k+1])).  view_use (may be NULL: all) masks views out: a pair with a    */
/*               masked-out view contributes nothing (the tool masks the views without a pose or an intrinsic).         */
/*   components  union of the two nodes of every match; a component's label is its smallest node row.  Hooking with an   */
/*               integer atomicMin on roots plus pointer jumping until a pass changes nothing: the fixed point does not  */
/*               depend on scheduling, two runs give the same arrays.  A match listed twice counts once.                 */
/*   filter      a component with two different features of one view is dropped whole (OpenMVG's conflict rule); then   */
/*               a component with fewer than min_length nodes (the tools pass 2; 0 counts as 1); a node no match        */
/*               touches is not a track.                                                                                */
/*   order       track ids 0, 1, 2, ... in ascending label; inside a track the observations ascend by view, which is    */
/*               ascending node row.  (OpenMVG numbers tracks by union-find root, which is not reproducible; every       */
/*               consumer in the reference renumbers.)                                                                   */
/*   errors      all checked before anything is launched: a view index out of range, a pair naming one view twice, a    */
/*               feature index out of range (the text names the pair and the match): SFMLOC_EINVAL; more than 2^32 - 2  */
/*               feature rows or matches: SFMLOC_ECAP.                                                                   */
/* sfmloc_sfm_triangulate (SfM_Data_Structure_Computation_Robust / _Blind) works on the handle's observations, poses    */
/* and intrinsics, and overwrites the resident X and the keep masks; sfmloc_sfm_clean, sfmloc_sfm_adjust[_joint],       */
/* sfmloc_sfm_read and sfmloc_sfm_read_structure follow on the same handle as after a cleanup (a later cleanup works on */
/* what was kept).  The handle may hold tracks with landmark_X all zero, or a map whose structure is to be rebuilt.      */
/* Per landmark, f64, unfused, only + - * / sqrt:                                                                        */
/*   posed       n = the observations whose view has a valid pose; the others are not kept and otherwise ignored (no    */
/*               GetPoseOrDie here).  n < 2: the landmark fails ("too few posed observations").                          */
/*   ray         the pixel is undistorted with get_ud_pixel (the bisection of "angle" above) for pinhole_radial_k3.     */
/*   projection  P = K [R | t], t_i = -((R_i0 C0 + R_i1 C1) + R_i2 C2): P_0j = f M_0j + ppx M_2j, P_1j = f M_1j +       */
/*               ppy M_2j, P_2j = M_2j with M = [R | t].                                                                 */
/*   hypothesis  two views: G = A^T A of the four rows x P_2 - P_0, y P_2 - P_1 ((x, y) the undistorted pixel), upper   */
/*               triangle, from 0.0, per observation G_ij = (G_ij + a_i a_j) + b_i b_j in list order, mirrored; the     */
/*               cyclic Jacobi of "jacobi" (sfmloc_merge section; 10 sweeps); the eigenvector of the smallest diagonal  */
/*               entry (the first on ties), divided by its w.  A zero or non-finite w or a non-finite point: no         */
/*               hypothesis.                                                                                             */
/*   rounds      mode SFMLOC_TRI_ROBUST: 2 n rounds, round r draws 2 distinct positions of the posed list with           */
/*               ac_sample<2> (Philox4x32-10 keyed by params.seed, stage 5, stream = the landmark's id, iteration r):   */
/*               a landmark's result does not depend on the batch.  n = 2: one round, the pair itself.                   */
/*   inliers     of a point: the posed observations with depth Xc_2 > 0 and sqrt(ex ex + ey ey) <= residual_px, the     */
/*               arithmetic of "residual" above, distortion applied, against the raw pixel.  A NaN is no inlier.         */
/*   winner      the round with the most inliers; on a tie the smaller sum of the inliers' ex ex + ey ey (added in list */
/*               order from 0.0); on a further tie the earlier round.  No round with a hypothesis: the landmark fails   */
/*               ("no valid hypothesis").                                                                                */
/*   final point G over the winner's inliers in list order (fewer than 2: "too few inliers"), the same eigen-solve (no  */
/*               point: "no valid hypothesis"), and its inliers evaluated once.                                          */
/*   keep rule   kept when the final inliers number at least min_inliers, or 2 when n = 2 and allow_pairs; otherwise     */
/*               "too few inliers".  A kept landmark's obs_keep is its final inlier mask; a failed landmark has X = 0,   */
/*               landmark_keep 0 and no observation kept.                                                                */
/*   blind       mode SFMLOC_TRI_BLIND: no rounds; G over every posed observation, then "inliers" with the depth test   */
/*               only, and the same keep rule.                                                                           */
/* No float atomics, no order-dependent atomics: two runs give the same bits.                                            */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_tracks sfmloc_tracks;
int sfmloc_tracks_build(int device, const uint64_t *view_off /*[n_views+1]*/, uint32_t n_views,
                        const uint8_t *view_use /*[n_views] or NULL*/, const uint32_t *pairs, uint32_t n_pairs,
                        const uint64_t *offsets, const uint32_t *match_i, const uint32_t *match_j, uint32_t min_length,
                        sfmloc_tracks **out);
/* components, dropped for conflict, dropped for length, kept (= the number of tracks) */
int sfmloc_tracks_counts(const sfmloc_tracks *t, uint64_t *counts /*[4]*/);
/* off [n_tracks+1] (sfmloc_tracks_counts gives n_tracks; off may be read alone first), view index and feature index of
 * every observation [off[n_tracks]]; any pointer may be NULL */
int sfmloc_tracks_read(const sfmloc_tracks *t, uint64_t *off, uint32_t *view, uint32_t *feat);
void sfmloc_tracks_destroy(sfmloc_tracks *t);
/* device milliseconds of the calling thread's last sfmloc_tracks_build (HIP events around its kernels and copies) */
double sfmloc_tracks_last_ms(void);

enum { SFMLOC_TRI_ROBUST = 0, SFMLOC_TRI_BLIND = 1 };
typedef struct sfmloc_triangulate_options {
  uint32_t mode;         /* SFMLOC_TRI_ROBUST (default) or SFMLOC_TRI_BLIND */
  uint32_t min_inliers;  /* default 3 (at least 2) */
  uint32_t allow_pairs;  /* default 1: a landmark with two posed observations is kept on 2 inliers */
  uint32_t reserved;
  double residual_px;    /* default 4.0 */
} sfmloc_triangulate_options;
typedef struct sfmloc_triangulate_report {
  uint64_t landmarks_in, landmarks_kept;
  uint64_t failed_posed, failed_hypothesis, failed_inliers; /* too few posed observations / no valid hypothesis / too few inliers */
  uint64_t obs_in, obs_kept;
  uint64_t rounds;       /* rounds run, all landmarks together */
  double device_ms;      /* HIP events around the call's kernels */
} sfmloc_triangulate_report;
void sfmloc_triangulate_default_options(sfmloc_triangulate_options *o);
/* opt NULL = the defaults; rep may be NULL */
int sfmloc_sfm_triangulate(sfmloc_sfm *h, const sfmloc_triangulate_options *opt, sfmloc_triangulate_report *rep);

/* ------------------------------------------------------------------------- */
/* Growing a map (sfmloc_sfm_register): the views the global chain left without a pose are resected against the kept     */
/* structure, the structure takes in their observations and the landmarks they make triangulable, round after round.     */
/* The growth step of incremental SfM, seeded by a structure that exists: the handle's keep masks must exist (after      */
/* sfmloc_sfm_triangulate or sfmloc_sfm_clean; SFMLOC_EINVAL before).  The reference has no such step (it rebuilds the  */
/* left-over frames as a map of their own and merges, cleanSfM + sfmMergeGraph): every rule below is a reading chosen    */
/* here, and tests/register_np.py restates each operation.  A round sees the poses, X and the masks as they stood when  */
/* it began, so its results do not depend on the order of its views.  A round, in this order:                            */
/*   count       c[v] = the observations of view v whose landmark is kept; the observation's own keep bit does not       */
/*               matter (an unposed view's observations are all unkept).                                                 */
/*   candidates  a view whose id_pose has no valid pose, with c[v] > min_points (MINIMUM_VIEW_NUM_TO_ESTIMATAE_CAMERA_   */
/*               POSE and its test ">", as sfmloc_sfm_resect), and either never tried on this handle or with c[v] larger */
/*               than at its last try: a failed view with an unchanged list would repeat its result exactly, the stream  */
/*               being its own id.  c[v] > 65 536: SFMLOC_ECAP, the "limit" of sfmloc_sfm_resect.  No candidate: the     */
/*               call ends, and this is not a round.                                                                     */
/*   list        the view's correspondences are its per-view list ("views" of sfmloc_sfm_resect: ascending landmark id)  */
/*               compacted to the kept landmarks, (pixel, X).  The pixel is undistorted with get_ud_pixel (the bisection */
/*               of "angle") for pinhole_radial_k3 and raw for pinhole: not the "raw pixels" quirk of sfmloc_sfm_resect, */
/*               which stays as it is.                                                                                   */
/*   resection   K5 as sfmloc_sfm_resect runs it: 32 views per gang session, the sampling stream = id_view, K = (f, ppx, */
/*               ppy) of the view's intrinsic, params.p3p_max_iteration.  Accepted when K5 reports ok (>= 8 inliers) and, */
/*               with min_inliers > 0, n_inliers >= min_inliers.  pose[id_pose] = Pose3(R, -R^T t) of KRt_From_P(P);     */
/*               two accepted views of one round sharing an id_pose: the last in ascending id wins ("success").  A view  */
/*               that is not accepted stays without a pose.                                                              */
/*   extend      every unkept observation of a kept landmark in a view registered this round becomes kept iff it passes  */
/*               "inliers" of sfmloc_sfm_triangulate at residual_px (depth > 0, the residual with the distortion applied */
/*               against the raw pixel, the arithmetic of "residual").  X does not move.                                 */
/*   landmarks   a landmark that is not kept, has an observation in a view registered this round and now has at least 2 */
/*               posed observations is triangulated by the per-landmark procedure of sfmloc_sfm_triangulate, robust     */
/*               mode, stream = its id, with tri_min_inliers, tri_allow_pairs and residual_px: its X, keep bits and      */
/*               landmark_keep are what a full sfmloc_sfm_triangulate would give it from the same poses (a failure       */
/*               leaves X = 0 and nothing kept).  No other landmark is touched.                                          */
/*   stop        after a round that registers no view, or after max_rounds rounds of this call.  Rounds are numbered     */
/*               over the handle's life: a later call goes on where the earlier one stopped, so max_rounds = 1 called k  */
/*               times equals one call with max_rounds = k.                                                              */
/* The call never changes the pose of a view that had one at entry, X or landmark_keep of a landmark kept at entry, or   */
/* the keep bit of an observation in a view posed at entry.  sfmloc_sfm_read, sfmloc_sfm_clean and the adjustments see   */
/* the new poses.  No float atomics and no order-dependent atomics: two runs give the same bits, and a handle that holds */
/* a subset of the candidate views with the same structure gives those views the same first-round results.               */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_register_options {
  uint32_t max_rounds;       /* default 16; 0 = until a round registers no view */
  uint32_t min_points;       /* default 10: a view is tried when it has MORE correspondences than this */
  uint32_t min_inliers;      /* default 0: K5's own gate (>= 8 inliers) alone; else n_inliers >= this as well */
  uint32_t tri_min_inliers;  /* default 3 (at least 2) */
  uint32_t tri_allow_pairs;  /* default 1 */
  uint32_t reserved;
  double residual_px;        /* default 4.0 */
} sfmloc_register_options;
typedef struct sfmloc_register_report {
  uint32_t rounds, views_unposed_in, views_tried, views_registered; /* of this call; views_tried counts every try */
  uint64_t obs_extended, landmarks_tried, landmarks_added;
  double device_ms;          /* HIP events on the handle's stream around the call, the waits between rounds included */
} sfmloc_register_report;
void sfmloc_register_default_options(sfmloc_register_options *o);
/* opt NULL = the defaults; rep may be NULL */
int sfmloc_sfm_register(sfmloc_sfm *h, const sfmloc_register_options *opt, sfmloc_register_report *rep);
/* per view: the result of the LAST round that tried it (zeros if never tried; n_obs = c[v] of that round, R and center
 * only when accepted); round[k] = that round or -1.  Either pointer may be NULL */
int sfmloc_sfm_register_read(const sfmloc_sfm *h, sfmloc_sfm_view_result *out /*[n_views]*/, int32_t *round /*[n_views]*/);
/* inliers of view k as indices into the correspondence list of the round that tried it last, AC-RANSAC order (as
 * sfmloc_sfm_resect_inliers: a failed view's best model included) */
int sfmloc_sfm_register_inliers(const sfmloc_sfm *h, uint32_t k, uint32_t *idx, uint32_t cap, uint32_t *n);
/* "count" of a round as it would stand now, for every view (posed or not): c[v] = the observations of view v whose
 * landmark is kept.  Read-only: nothing on the handle changes, no round is counted.  SFMLOC_EINVAL before the keep
 * masks exist.  What a driver needs for OpenMVG's "views close to the best" rule (sfmlocalization_amd.incrementalsfm) */
int sfmloc_sfm_register_counts(const sfmloc_sfm *h, uint32_t *c /*[n_views]*/);

/* ------------------------------------------------------------------------- */
/* Relative poses (the first stage of openMVG_main_GlobalSfM, reconstructGraph.py:166-171: the essential matrix of      */
/* every matched view pair by the five-point solver under AC-RANSAC, its decomposition and the cheirality test).        */
/* Rotation and translation averaging consume the result ("Global poses" below); OpenMVG's two-view bundle adjustment  */
/* of the winning pose is a call of its own ("Two-view refinement" below): here R and t are the winning sample's.       */
/* OpenMVG's source was not at hand: every point below is a reading chosen here, and                                    */
/* tests/relpose_np.py restates each operation.  The pair list has the layout of sfmloc_geometric_pairs and             */
/* sfmloc_tracks_build (pair k = views (I, J) = (pairs[2k], pairs[2k+1]) owns match_i/j[offsets[k] .. offsets[k+1]),    */
/* feature indices inside the view); kpt_xy [view_off[n_views] * 2] the keypoints of all views; intrinsics f, ppx, ppy, */
/* k1, k2, k3 with type 0 (pinhole) or 3 (pinhole_radial_k3).  Per pair, f64, unfused, only + - * / sqrt:               */
/*   bearings    the pixel undistorted with get_ud_pixel ("angle" above) when the view's intrinsic is type 3, then      */
/*               ((x - ppx) / f, (y - ppy) / f).  The two views may have different intrinsics.                           */
/*   gate        m <= 5 matches: ok = 0, every other field but n_matches zero, no error.                                 */
/*   sample      five distinct sorted positions by OpenMVG's UniformSample (the insertion of ac_sample) from            */
/*               Philox4x32-10 keyed by the seed's two halves with the counter (iteration, I, J, 6 | (d >> 2) << 8), d   */
/*               the draw 0 .. 4 and word d & 3 of the block its value (6: the stage id).  I and J are the call's view  */
/*               indices: a pair's result depends on (seed, I, J) and its own matches alone, not on the other pairs.    */
/*   solver      design matrix D [5 x 9], row (u a, u b, u, v a, v b, v, a, b, 1) for the bearings (a, b) in I and       */
/*               (u, v) in J; G = D^T D, rows added in order; "jacobi" (sfmloc_merge section, N = 9, 10 sweeps).  X, Y,  */
/*               Z, W = the eigenvectors of the four smallest diagonal entries in ascending order, each time the first  */
/*               smallest entry not yet taken; no model when the fifth smallest <= 1e-12 * the largest (a repeated      */
/*               point).  E = x X + y Y + z Z + W row-major.  The ten cubics -- det E, and the nine entries of          */
/*               (E E^T - tr(E E^T) / 2) E -- in the monomial order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz */
/*               x yz^2 yz y z^3 z^2 z 1 (products of linear forms accumulated from 0.0 term by term, csrc/             */
/*               essential_device.h); Gauss-Jordan on the first ten columns with partial pivoting (the largest          */
/*               magnitude, the first on ties; a pivot not above 1e-13 in magnitude: no model).  Nister's route: rows   */
/*               4 .. 9 pairwise as a - z b give the 3 x 3 matrix of polynomials in z (degrees 3, 3, 4), its            */
/*               determinant p of degree 10.  Real roots: the Sturm chain of p / max|p_i| (every member divided by its  */
/*               largest magnitude), the Cauchy bound 1 + max |p_i / p_10|, the k-th root by 48 bisections on the       */
/*               chain's sign-change count, then 3 Newton steps each kept only inside the last bracket, then 2 Newton   */
/*               steps on the determinant of the matrix itself (entries by Horner, the derivative as the sum of the    */
/*               three determinants with one row differentiated), each kept when |dz| <= 1e-6 (1 + |z|).  x, y from the */
/*               cross product of two rows of the matrix at z (of the three pairs the one with the largest third        */
/*               entry, the first on ties).  Each model is scaled to unit Frobenius norm; a non-finite one is dropped.  */
/*               Up to 10 models, in ascending z.                                                                        */
/*   residual    the squared distance in J's undistorted pixels from the point to the line E x_I: the arithmetic of     */
/*               the F-matrix residual on bearings ((l u)^2 / (l0^2 + l1^2), NaN -> +inf), times f_J f_J.               */
/*   NFA         logalpha0 = log10(2 D / A) of image J (D the diagonal, A the area, pixels), mult 0.5, loge0 =          */
/*               log10(10 (m - 5)), upper bound precision_px^2 (+inf: none); the logcombi tables in float as K3's.      */
/*   AC-RANSAC   K3's loop (OpenMVG ACRANSAC): max_iteration less a 10 % reserve, residuals sorted by (error, index),   */
/*               a better NFA below 0 (or the last planned iteration) restricts sampling to the inlier set and spends   */
/*               the reserve.  The models of an iteration are tried in ascending z.                                      */
/*   decision    nfa >= 0 or no model at all: n_inliers = 0, ok = 0, nfa reported, the rest zero.  Otherwise every      */
/*               field is filled and ok = (n_inliers > 2.5 * 5) and front[choice] > 0.  error_max_px = the square root  */
/*               of the last inlier's residual.  The inlier list is in AC-RANSAC's order (ascending residual).          */
/*               ok does not say that every inlier lies in front: a pair without a baseline (pure rotation) has its     */
/*               points at infinity, the sign of a depth is then the noise's, and it may end ok with front[choice] <    */
/*               n_inliers.  A consumer that needs the translation checks front[choice] against n_inliers.              */
/*   decompose   "jacobi" (N = 3) on E^T E; v1, v2 the columns of the largest and second largest diagonal entry (the    */
/*               first on ties), sigma_i its square root, u_i = E v_i / sigma_i, v3 = v1 x v2, u3 = u1 x u2 scaled to   */
/*               unit length (so det U = det V = +1).  Ra = U W V^T = u2 v1^T - u1 v2^T + u3 v3^T, Rb = U W^T V^T =     */
/*               u1 v2^T - u2 v1^T + u3 v3^T.  Candidates 0 .. 3: (Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3).             */
/*   cheirality  every inlier triangulated from [I | 0] and [R | t] on bearings by "hypothesis" of the structure        */
/*               section (4 x 4 G, Jacobi, the smallest diagonal entry); front[c] counts those with a point and         */
/*               X_2 > 0 and (R X + t)_2 > 0.  choice = the largest count, the first on ties.                            */
/* Pairs of at most 2048 matches run with their arrays in LDS, larger ones (at most 65 536: SFMLOC_ECAP beyond) through  */
/* global-memory slots with the same arithmetic and bits.  No float atomics: two runs give the same bits.  Errors, all   */
/* checked before anything is launched: a view or intrinsic index out of range, a pair naming one view twice, a feature  */
/* index out of range (the text names the pair and the match), an intrinsic type other than 0 or 3: SFMLOC_EINVAL.      */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_relpose sfmloc_relpose;
typedef struct sfmloc_relpose_options {
  uint32_t max_iteration;   /* default 256 */
  uint32_t reserved;
  double   precision_px;    /* AC-RANSAC upper bound on the residual, default 2.5; +inf = none */
  uint64_t seed;            /* default: sfmloc_default_params' seed */
} sfmloc_relpose_options;
typedef struct sfmloc_relpose_result {
  uint32_t ok, n_matches, n_inliers;
  uint32_t sample[5];        /* positions in the pair's match list of the winning minimal sample */
  uint32_t front[4];         /* inliers in front of both cameras, per decomposition candidate */
  uint32_t choice;           /* index of the chosen candidate */
  double   E[9], R[9], t[3]; /* x_J^T E x_I = 0 on bearings; X_J = R X_I + t, |t| = 1 */
  double   error_max_px, nfa;
} sfmloc_relpose_result;
void sfmloc_relpose_default_options(sfmloc_relpose_options *o);
/* opt NULL = the defaults; n_pairs = 0 gives an empty handle */
int  sfmloc_relative_poses(int device, const uint64_t *view_off /*[n_views+1]*/, uint32_t n_views, const float *kpt_xy,
                           const uint32_t *view_wh /*[n_views*2]*/, const uint32_t *view_intrinsic /*[n_views]*/,
                           const double *intrinsics /*[n*6]*/, const uint32_t *intrinsic_type, uint32_t n_intrinsics,
                           const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                           const uint32_t *match_i, const uint32_t *match_j,
                           const sfmloc_relpose_options *opt, sfmloc_relpose **out);
int  sfmloc_relpose_results(const sfmloc_relpose *r, sfmloc_relpose_result *out /*[n_pairs]*/);
/* off [n_pairs+1], idx [off[n_pairs]]: positions in each pair's match list, AC-RANSAC's order; either may be NULL */
int  sfmloc_relpose_inliers(const sfmloc_relpose *r, uint64_t *off /*[n_pairs+1]*/, uint32_t *idx);
void sfmloc_relpose_destroy(sfmloc_relpose *r);
/* device milliseconds of the calling thread's last sfmloc_relative_poses (HIP events around its kernels and copies) */
double sfmloc_relpose_last_ms(void);
/* parity probe of the solver alone: a row = x1[10], x2[10] (five bearing pairs); out [n * 91] = count, then up to 10 E */
int  sfmloc_debug_five_point(int device, const double *in, int n, double *out);

/* ------------------------------------------------------------------------- */
/* Two-view refinement (what OpenMVG does to every relative pose before it averages them: the pose of the winning       */
/* minimal sample is adjusted on all of the pair's inliers).  An opt-in stage after sfmloc_relative_poses: per pair it   */
/* minimises the reprojection error of the inlier matches over the relative pose and the matches' 3D points, one         */
/* workgroup of 256 threads per pair, the points eliminated as the joint bundle adjustment eliminates landmarks.  The    */
/* arrays are those of sfmloc_relative_poses (view_wh is not needed), rel_R / rel_t and inlier_off / inlier_idx its      */
/* results, use_pair[k] = 0 (NULL: all 1) leaves a pair as it is.  OpenMVG's source was not at hand: every point below   */
/* is a reading chosen here, and tests/relrefine_np.py restates each operation.  f64, unfused, only + - * / sqrt:        */
/*   bearings    as "bearings" of the relative poses, for the inlier matches only.                                       */
/*   points      every inlier is triangulated from [I | 0] and [R | t] by "cheirality" of the relative poses.  It is     */
/*               used when the point X exists, (R X + t)_2 is finite and X_2 and (R X + t)_2 are positive.  A match      */
/*               listed twice is two used points.  n_used counts the used inliers.                                       */
/*   status      0: use_pair was 0.  2: n_used < min_points.  4: no step was ever accepted, or a sum of the first        */
/*               linearisation was not finite.  In these three R and t are copies of the inputs and steps counts the     */
/*               steps tried (0 for 0 and 2); cost_initial and cost are 0 for 0 and 2 and for a first linearisation      */
/*               that was not finite.  1: stopped by the rule of "step".  3: max_steps were tried; the last accepted     */
/*               pose is kept.  Always E = [t]x R of the R and t returned, divided by its Frobenius norm (the nine       */
/*               squares added in row-major order); all zero where that norm is zero.                                    */
/*   residual    four values per used inlier, in undistorted pixels: f_I (X_xy / X_2 - b_I) and f_J (Y_xy / Y_2 - b_J),  */
/*               Y = R X + t, b the bearings, f the focal lengths of the two views' intrinsics.  No robust loss: the     */
/*               inliers are already selected.  cost = 1/2 sum r^2, r^2 = ((r0^2 + r1^2) + r2^2) + r3^2 per inlier.      */
/*   parameters  the rotation moves by R <- C(w) R, C(w) = I + 2 / (1 + w.w) ([w]x + w w^T - (w.w) I) (Cayley, as the    */
/*               rotation averaging); the translation on the unit sphere by t <- (t + B d) / |t + B d|, B [3 x 2] the     */
/*               tangent basis b1 = (t x e_k) / |t x e_k|, b2 = t x b1, k the axis of the smallest |t_k|, the first on    */
/*               ties; three values per point.  Derivatives to first order: dY/dw = -2 [R X]x, dY/dd = B, dY/dX = R.     */
/*   step        the lane that owns a point forms its block V = Jx^T Jx [3 x 3], its coupling W = Jp^T Jx [5 x 3], its   */
/*               gradient Jx^T r and its part of Jp^T Jp and Jp^T r (Jp the 2 x 5 derivative of the second view's two   */
/*               residuals by (w, d)).  Vd = V + lambda clamp(diag V, 1e-6, 1e32), inverted by Cholesky.  The reduced    */
/*               system is A = sum (Jp^T Jp - W Vd^-1 W^T), g = sum (Jp^T r - W Vd^-1 Jx^T r), the difference taken per  */
/*               point; (A + lambda clamp(diag A, 1e-6, 1e32)) x = -g by Cholesky on thread 0, broadcast through LDS     */
/*               (ba_solve<5> of csrc/ba_device.h, which also gives the decrease the model promises).  The point's step  */
/*               is -Vd^-1 (Jx^T r + W^T x).  The trial is costed anew at the trial pose and trial points; it is taken   */
/*               when every used point has finite positive depth in both views there, the cost is finite and lower and   */
/*               the decrease is above 1e-3 of the promised one.  lambda starts at 1e-4; acceptance, rejection and the   */
/*               stopping rule (relative decrease <= 1e-14, the promise itself below that, or lambda >= 1e32) are those  */
/*               of the separable bundle adjustment (BaLm of csrc/ba_device.h).  steps counts the trials.                */
/*   reduction   lane l of the 256 adds its points l, l + 256, ... in ascending order from 0; then the butterfly over    */
/*               the wave's 64 lanes (xor 32, 16, .. 1); then every thread adds the four waves' sums in the order 0 .. 3. */
/* One form serves any inlier count: bearings, points and trial points live in global memory, one slab per pair at the   */
/* pair's inlier offset, component by component (lane-consecutive addresses).  Device memory: 80 bytes per inlier        */
/* (bearings 32, points 24, trial points 24) beside the call's input arrays; a failed allocation is SFMLOC_ENOMEM.      */
/* No float atomics: two runs give the same bits, and a pair's record depends on its own inputs alone, not on the other */
/* pairs or on the order of the pair list.  Refusals, all on the host before any launch, the text naming the pair:      */
/* everything sfmloc_wedge_scales refuses for these arrays; max_steps = 0, min_points < 6: SFMLOC_EINVAL.               */
/* n_pairs = 0 gives an empty handle.                                                                                    */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_relrefine sfmloc_relrefine;
typedef struct sfmloc_relrefine_options {
  uint32_t max_steps;    /* default 100 */
  uint32_t min_points;   /* default 13: the smallest count above 2.5 x 5, the gate of sfmloc_relpose_result.ok */
} sfmloc_relrefine_options;
typedef struct sfmloc_relrefine_result {
  uint32_t status, n_used, steps, reserved;
  double   R[9], t[3], E[9];   /* X_J = R X_I + t, |t| = 1; E = [t]x R at unit Frobenius norm */
  double   cost_initial, cost; /* 1/2 sum r^2 over the used inliers, pixels^2 */
} sfmloc_relrefine_result;
void sfmloc_relrefine_default_options(sfmloc_relrefine_options *o);
/* opt NULL = the defaults */
int  sfmloc_refine_relative_poses(int device, const uint64_t *view_off /*[n_views+1]*/, uint32_t n_views,
                                  const float *kpt_xy, const uint32_t *view_intrinsic /*[n_views]*/,
                                  const double *intrinsics /*[n*6]*/, const uint32_t *intrinsic_type,
                                  uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                                  const uint32_t *match_i, const uint32_t *match_j,
                                  const double *rel_R /*[n_pairs*9]*/, const double *rel_t /*[n_pairs*3]*/,
                                  const uint64_t *inlier_off /*[n_pairs+1]*/, const uint32_t *inlier_idx,
                                  const uint8_t *use_pair /*[n_pairs], NULL = all*/,
                                  const sfmloc_relrefine_options *opt, sfmloc_relrefine **out);
int  sfmloc_relrefine_results(const sfmloc_relrefine *r, sfmloc_relrefine_result *out /*[n_pairs]*/);
void sfmloc_relrefine_destroy(sfmloc_relrefine *r);
/* device milliseconds of the calling thread's last sfmloc_refine_relative_poses */
double sfmloc_relrefine_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Wedge scales (the ratio of two pair baselines from the depths of the features the pairs share: what fixes the        */
/* spacing of cameras along a line, where pairwise directions say nothing; OpenMVG gets it from triplet translations).  */
/* A wedge is two pairs k < l of the pair list that share a view v.  The arrays are those of sfmloc_relative_poses      */
/* (view_wh is not needed), rel_R / rel_t and inlier_off / inlier_idx its results (sfmloc_relpose_result's R, t;        */
/* sfmloc_relpose_inliers), use_pair[k] = 0 (NULL: all 1) leaves a pair out.  tests/pairscales_np.py restates every     */
/* operation.  f64, unfused, only + - * / sqrt:                                                                          */
/*   bearings    as "bearings" of the relative poses, for the inlier matches only.                                       */
/*   depths      every inlier match of a used pair is triangulated from [I | 0] and [R | t] by "cheirality" of the       */
/*               relative poses.  It yields z_I = X_2 and z_J = (R X + t)_2 when the point exists, z_J is finite and     */
/*               both are positive; otherwise nothing.                                                                    */
/*   lists       per pair and side, the yielded depths keyed by the feature index in that side's view, ascending by      */
/*               feature.  Of the yielding matches of a pair that name the same feature of a view, the first in the      */
/*               order of the inlier list is kept (each side decides for itself).  Built by two stable radix sorts of    */
/*               all (pair side, feature) entries at once (csrc/radix_sort.h), so a pair may have any number of inliers. */
/*   candidates  per view, its used pairs ascending by pair index (built on the host); every two of them are a           */
/*               candidate.  A view of at most 64 pairs is enumerated by one lane, a larger one by one wave.             */
/*   count       one wave per candidate: the features of the shorter of v's two lists are looked up in the longer by     */
/*               binary search; n_shared = the features in both.  A candidate with n_shared < min_shared is not emitted. */
/*               The others are compacted (flag, scan, scatter) and ordered by (k, l, view) by three stable radix sorts.  */
/*   ratio       one workgroup per record: the shared features in ascending feature order, the first max_shared of them, */
/*               give q_f = z_k(f) / z_l(f) (the depths of f in view v); ratio = the lower median of q in the order      */
/*               (value, feature), element (n - 1) / 2 of n, sorted in LDS.  It estimates b_l / b_k, the two baselines   */
/*               in one unit, since rel_t has unit length in both pairs.  n_shared reports all shared features, also     */
/*               beyond max_shared.                                                                                       */
/* No float atomics; nothing but a selection follows the depths: two runs give the same bits, and a record does not      */
/* depend on the other pairs or on the order of the pair list (which only decides which pair of a wedge is k).           */
/* Refusals, all on the host before any launch, the text naming the pair: every check of sfmloc_relative_poses, an       */
/* inlier position out of its pair's range, inlier offsets that are not monotone, a non-finite rel_R or rel_t,           */
/* min_shared < 1, max_shared outside 1 .. 2048: SFMLOC_EINVAL; 2^30 pairs, more than 2^31 - 1024 inliers or candidates: */
/* SFMLOC_ECAP.                                                                                                           */
/* n_pairs = 0 gives an empty handle.  Consumer: sfmloc_global_poses_scaled ("Scaled global poses" below).              */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_wscales sfmloc_wscales;
typedef struct sfmloc_wscales_options {
  uint32_t min_shared;   /* default 8 */
  uint32_t max_shared;   /* default 2048, which is also the most */
} sfmloc_wscales_options;
typedef struct sfmloc_wscale {
  uint32_t view, k, l, n_shared;   /* k < l: positions in the pair list */
  double   ratio;                  /* b_l / b_k */
} sfmloc_wscale;
typedef struct sfmloc_wscales_report {
  uint32_t n_pairs, n_pairs_used;
  uint32_t n_inliers;      /* inlier matches of the used pairs */
  uint32_t n_depths;       /* of them, the ones that yield depths */
  uint32_t n_candidates, n_wedges;
  uint32_t launches, reserved;
  double   device_ms;      /* HIP events around the call's kernels and copies */
} sfmloc_wscales_report;
void sfmloc_wscales_default_options(sfmloc_wscales_options *o);
/* opt NULL = the defaults */
int  sfmloc_wedge_scales(int device, const uint64_t *view_off /*[n_views+1]*/, uint32_t n_views, const float *kpt_xy,
                         const uint32_t *view_intrinsic /*[n_views]*/, const double *intrinsics /*[n*6]*/,
                         const uint32_t *intrinsic_type, uint32_t n_intrinsics,
                         const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                         const uint32_t *match_i, const uint32_t *match_j,
                         const double *rel_R /*[n_pairs*9]*/, const double *rel_t /*[n_pairs*3]*/,
                         const uint64_t *inlier_off /*[n_pairs+1]*/, const uint32_t *inlier_idx,
                         const uint8_t *use_pair /*[n_pairs], NULL = all*/,
                         const sfmloc_wscales_options *opt, sfmloc_wscales **out);
int  sfmloc_wscales_count(const sfmloc_wscales *w, uint32_t *n_wedges);
int  sfmloc_wscales_read(const sfmloc_wscales *w, sfmloc_wscale *out /*[n_wedges]*/);
int  sfmloc_wscales_report_read(const sfmloc_wscales *w, sfmloc_wscales_report *rep);
void sfmloc_wscales_destroy(sfmloc_wscales *w);
/* device milliseconds of the calling thread's last sfmloc_wedge_scales */
double sfmloc_wscales_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Seed scores (the initial pair of incremental SfM, OpenMVG's AutomaticInitialPairChoice: per matched pair the median  */
/* angle between the two rays of its inlier matches; the pair with the largest one starts the map).  The arrays are     */
/* those of sfmloc_wedge_scales: the scene of sfmloc_relative_poses (view_wh is not needed), rel_R / rel_t and          */
/* inlier_off / inlier_idx its results, use_pair[k] = 0 (NULL: all 1) leaves a pair out.  OpenMVG's source was not at   */
/* hand: every point below is a reading chosen here, and tests/seed_np.py restates each operation.  Per used pair, f64, */
/* unfused, only + - * / sqrt:                                                                                           */
/*   bearings    as "bearings" of the relative poses, for the inlier matches, in the order of the inlier list.           */
/*   point       every inlier is triangulated from [I | 0] and [R | t] by "cheirality" of the relative poses.  It is     */
/*               used under the rule of "points" of the two-view refinement: the point X exists, (R X + t)_2 is finite   */
/*               and X_2 and (R X + t)_2 are positive.  A match listed twice is two used inliers.                         */
/*   cosine      r1 = (u_I, v_I, 1), r2 = R^T (u_J, v_J, 1) (each component (R_0c u + R_1c v) + R_2c), the bearings of   */
/*               the match; c = dot / (|r1| |r2|), dot and the squared norms summed x, y, z in order, |r| = sqrt.  c is  */
/*               clamped as "angle" of sfmloc_sfm_clean clamps: max(lo, min(c, hi)), lo = -1 + 1e-8, hi = 1 - 1e-8, a    */
/*               NaN cosine becomes lo.                                                                                   */
/*   key         the cosine's 64 bits as an unsigned key that orders doubles ascending: all bits flipped when the sign   */
/*               bit is set, the top bit set otherwise.  Order is by key: -0.0 comes before +0.0.                        */
/*   median      of the n_used keys in DESCENDING order, the element of rank n_used / 2 counted from 0 (OpenMVG's        */
/*               nth_element index on ascending angles).  cos_median = that element's double; 0.0 when n_used = 0.       */
/*   record      candidate = n_used >= min_used && cos_median < max_cos && cos_median > min_cos.  The thresholds are     */
/*               cosines: no acos runs on the device and no libm call stands between tests/seed_np.py and the kernel.    */
/*               A pair with use_pair = 0 has an all-zero record.                                                         */
/* One form serves any inlier count (a pair may hold 65 536): one workgroup of 256 threads per pair writes every         */
/* inlier's key, or 0 for one that is not used (no clamped cosine has the key 0), to a slab in global memory at the pair's */
/* inlier offset, 8 bytes per inlier, lane-consecutive; then a radix select, 8 passes of 8 bits from the top, a          */
/* 256-bin integer histogram in LDS per pass: the bin that holds the wanted rank narrows the prefix.  Integer LDS        */
/* atomics are order-free and a selection gives the same element whatever the order of ties: two runs give the same      */
/* bits, and a record depends on its own pair alone, not on the other pairs or on the order of the pair list.  No float  */
/* atomics.  Device memory: 8 bytes per inlier beside the call's input arrays.                                           */
/* Refusals, all on the host before any launch, the text naming the pair: everything sfmloc_wedge_scales refuses for    */
/* these arrays; min_used = 0, a threshold that is not finite or outside (-1, 1], min_cos >= max_cos: SFMLOC_EINVAL.     */
/* n_pairs = 0 gives an empty handle.  The choice among the candidates is the host's (csrc/seed_host.h choose, restated  */
/* by tests/seed_np.py): two views of different id_pose, the smallest cos_median, then the larger n_used, then the       */
/* smaller pair index.  Consumer: sfmlocalization_amd.incrementalsfm.                                                    */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_seed sfmloc_seed;
typedef struct sfmloc_seed_options {
  uint32_t min_used;     /* default 100 */
  uint32_t reserved;
  double   max_cos;      /* default cos 3 degrees = 0.9986295347545738: a smaller median angle is no baseline */
  double   min_cos;      /* default cos 60 degrees = 0.5 */
} sfmloc_seed_options;
typedef struct sfmloc_seed_score {
  uint32_t n_inliers, n_used, candidate, reserved;
  double   cos_median;
} sfmloc_seed_score;
void sfmloc_seed_default_options(sfmloc_seed_options *o);
/* opt NULL = the defaults */
int  sfmloc_seed_scores(int device, const uint64_t *view_off /*[n_views+1]*/, uint32_t n_views, const float *kpt_xy,
                        const uint32_t *view_intrinsic /*[n_views]*/, const double *intrinsics /*[n*6]*/,
                        const uint32_t *intrinsic_type, uint32_t n_intrinsics,
                        const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                        const uint32_t *match_i, const uint32_t *match_j,
                        const double *rel_R /*[n_pairs*9]*/, const double *rel_t /*[n_pairs*3]*/,
                        const uint64_t *inlier_off /*[n_pairs+1]*/, const uint32_t *inlier_idx,
                        const uint8_t *use_pair /*[n_pairs], NULL = all*/,
                        const sfmloc_seed_options *opt, sfmloc_seed **out);
int  sfmloc_seed_read(const sfmloc_seed *s, sfmloc_seed_score *out /*[n_pairs]*/);
void sfmloc_seed_destroy(sfmloc_seed *s);
/* device milliseconds of the calling thread's last sfmloc_seed_scores */
double sfmloc_seed_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Global poses (the middle stage of openMVG_main_GlobalSfM: rotation averaging and translation averaging over the     */
/* relative poses of the section above; its result is what "Structure from known poses" starts from).  OpenMVG's       */
/* source was not at hand: every point below is a reading chosen here, and tests/globalposes_np.py restates each one.   */
/* Pair k = views (I, J) = (pairs[2k], pairs[2k+1]) with rel_R[9k..] row-major and rel_t[3k..] in the convention of     */
/* sfmloc_relpose_result: X_J = R X_I + t, |t| = 1.  use_t[k] = 0 (NULL: all 1) keeps a pair's translation out (the     */
/* advice of "decision" above: front[choice] < n_inliers).  On the device f64, unfused, only + - * / sqrt; the host     */
/* computes the cosine of the triplet angle and the tangent of rotation_delta's default.                                */
/*   adjacency   CSR by view over both directions of every pair, a view's entries ascending by neighbour (built on the  */
/*               host).  Every sum over a view's pairs below runs in that order, so a result does not depend on the     */
/*               order of the pair list.  Views of more than 64 pairs are gathered by one wave each (lane-strided, then  */
/*               the six-level butterfly), the others by one lane each.                                                  */
/*   triplets    every triangle a < b < c of the pair graph.  R_xy = rel_R of the pair when it is stored as (x, y), its */
/*               transpose when stored as (y, x).  The cycle rotation is M = R_ca (R_bc R_ab); the triplet passes when  */
/*               trace M > 1 + 2 cos(triplet_angle_deg) (default 5 degrees, OpenMVG's).  One wave per pair intersects   */
/*               the two adjacency lists; n_triplets / n_triplets_ok of a pair count the triangles it lies in; nothing  */
/*               else of a triplet is stored (summed over the wave, integers).  kept = n_triplets_ok > 0.                 */
/*   component   connected components over the pairs with kept and use_t (the hook / pointer-jump kernels of            */
/*               sfmloc_tracks, csrc/graph_device.h).  The component with the most views wins, the one with the          */
/*               smallest view index on a tie; its smallest view is the root, R = I, C = 0.  No component of two views   */
/*               (no triplet passes): every in_component is 0, the report is filled, no error.  "rotation pairs" = kept  */
/*               pairs with both views in the component; "translation pairs" = the rotation pairs with use_t.            */
/*   chordal     minimise sum |R_j - R_ij R_i|_F^2 over the rotation pairs with the root fixed: per view, deg X_v -     */
/*               sum Off X_n = b_v, Off = R_ij in J's row and R_ij^T in I's, b_v = Off for the pair to the root.  One    */
/*               conjugate-gradient run on the 9 values per view together ("PCG" below, preconditioner 1 / deg).  Each  */
/*               X_v to the nearest rotation: "jacobi" (N = 3) on X^T X = V diag(l) V^T, R = X V diag(s_i / sqrt(l_i))   */
/*               V^T with s = 1, except s = -1 at the smallest l (the first on ties) when det X < 0.                     */
/*   IRLS        per rotation pair E = R_j^T (R_ij R_i), g = (E21 - E12, E02 - E20, E10 - E01) / (1 + tr E), |g| =       */
/*               tan(theta / 2); 1 + tr E <= 1e-12: weight 0, g = 0, no cost.  Huber in |g| with delta = rotation_delta */
/*               (default tan(triplet_angle / 6): half of a third of the triplet bound): w = 1, rho = |g|^2 / 2 up to   */
/*               delta, then w = delta / |g|, rho = delta (|g| - delta / 2).  Solve sum_e w (x_v - x_n) = sum +-w g     */
/*               (+ in J's row, - in I's), x_root = 0, by PCG (preconditioner 1 / sum w); R_v <- R_v (I + 2 / (1 + x.x)  */
/*               ([x]x + [x]x^2)).  A step whose robust cost is not lower is not applied and ends the loop (stop 2);    */
/*               stop 0 after an applied step with (cost - cost') <= function_tolerance * cost, or at cost 0 or a zero  */
/*               right-hand side; stop 1 after max_steps.                                                                */
/*   translation d = -R_j^T t_ij scaled to unit length: the world direction from C_i to C_j.  Per translation pair,     */
/*               D = C_j - C_i, s = d.D, r = D - max(1, s) d, Huber in |r| with translation_delta (default 0.05, in     */
/*               units of the bound s >= 1, which is what forbids the collapsed solution), block W = w (I - d d^T) when */
/*               s > 1, else w I.  Gauss-Newton under "solver" of the joint block (lambda 1e-4, D = diag clamped to     */
/*               [1e-6, 1e32], acceptance ratio 1e-3, the lambda update, "stopping"), from C = 0, C_root = 0: per view  */
/*               (sum W + lambda D) x_v - sum W x_n = -+w r, PCG with the inverse of the view's own 3 x 3 block; model  */
/*               decrease sum_e -(w r).u - u^T W u / 2, u = x_j - x_i.                                                  */
/*   PCG         from x = 0; stops at |r| <= pcg_tolerance |r0|, after max_pcg iterations, or when r.z or p.Ap is not   */
/*               positive.  Scalar products are per-workgroup partials summed by a fixed tree (store, then sum); costs  */
/*               are summed per view over the pairs to a larger neighbour, then the same way.  Iterations are queued 32 */
/*               at a time with one small read-back per chunk and per step; a finished solve makes the rest of its      */
/*               chunk return at once.  No float atomics: two runs give the same bits.                                   */
/* Known limit of this call: pairwise directions do not determine the spacing along a collinear stretch of cameras.    */
/* There only the bound s >= 1 and the Huber term act, and one bad pair can fold two centres together.                  */
/* sfmloc_global_poses_scaled ("Scaled global poses" below) fixes the spacing from the ratios of sfmloc_wedge_scales.    */
/* Refusals, all on the host before any launch, the text naming the pair: a view index out of range, a pair naming one  */
/* view twice, the same unordered pair listed twice, a non-finite entry, |R^T R - I| (largest entry) or | |t| - 1 |     */
/* above 1e-6: SFMLOC_EINVAL.  n_pairs = 0 gives an empty handle.                                                        */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_gposes sfmloc_gposes;
typedef struct sfmloc_gposes_options {
  double   triplet_angle_deg;   /* default 5 */
  double   rotation_delta;      /* Huber delta on |g| = tan(theta / 2); <= 0 (the default): tan(triplet_angle / 6) */
  double   translation_delta;   /* default 0.05 */
  double   function_tolerance;  /* default 1e-6, both loops */
  double   pcg_tolerance;       /* default 1e-6 */
  uint32_t max_steps;           /* default 50, both loops */
  uint32_t max_pcg;             /* default 20000 iterations per solve */
} sfmloc_gposes_options;
typedef struct sfmloc_gposes_pair {
  uint32_t n_triplets, n_triplets_ok, kept, used_t;  /* used_t: a translation pair */
  double   rot_residual;    /* |g| at the result, 0 unless a rotation pair */
  double   trans_residual;  /* |r| at the result, 0 unless a translation pair */
} sfmloc_gposes_pair;
typedef struct sfmloc_gposes_report {
  uint32_t n_views, n_pairs, n_triplets, n_triplets_ok, n_pairs_kept;
  uint32_t n_component_views, root, n_rotation_pairs, n_translation_pairs;
  uint32_t chordal_pcg, chordal_stop;            /* PCG stop: 0 tolerance, 1 max_pcg, 2 r.z or p.Ap not positive */
  uint32_t rot_steps_tried, rot_steps_accepted, rot_pcg_total, rot_stop;
  uint32_t trans_steps_tried, trans_steps_accepted, trans_pcg_total, trans_stop;  /* stop 2: lambda passed 1e32 */
  uint32_t launches;                             /* kernels queued by the call */
  double   chordal_residual;                     /* |r| / |r0| where the chordal PCG stopped */
  double   chordal_cost;                         /* sum |R_j - R_ij R_i|_F^2 over the rotation pairs at the projected start */
  double   rot_cost_initial, rot_cost_final;     /* the robust cost at the chordal start and at the result */
  double   trans_cost_initial, trans_cost_final;
  double   graph_ms, rotation_ms, translation_ms; /* device time of triplets + component, chordal + IRLS, translation */
  double   device_ms;                            /* HIP events around the call's kernels and copies */
} sfmloc_gposes_report;
void sfmloc_gposes_default_options(sfmloc_gposes_options *o);
/* opt NULL = the defaults */
int  sfmloc_global_poses(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs,
                         const double *rel_R /*[n_pairs*9]*/, const double *rel_t /*[n_pairs*3]*/,
                         const uint8_t *use_t /*[n_pairs], NULL = all*/,
                         const sfmloc_gposes_options *opt, sfmloc_gposes **out);
/* any of the three may be NULL; R and C of a view outside the component are zero */
int  sfmloc_gposes_views(const sfmloc_gposes *g, uint8_t *in_component /*[n]*/, double *R /*[n*9]*/, double *C /*[n*3]*/);
int  sfmloc_gposes_pairs(const sfmloc_gposes *g, sfmloc_gposes_pair *out /*[n_pairs]*/);
int  sfmloc_gposes_report_read(const sfmloc_gposes *g, sfmloc_gposes_report *rep);
void sfmloc_gposes_destroy(sfmloc_gposes *g);
/* device milliseconds of the calling thread's last sfmloc_global_poses */
double sfmloc_gposes_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Scaled global poses: sfmloc_global_poses with every translation pair's baseline fixed beforehand from the wedge      */
/* ratios of sfmloc_wedge_scales, so that cameras along a line keep their spacing.  The arguments of                    */
/* sfmloc_global_poses, then wedge w = pairs (k, l) = (wedge_kl[2w], wedge_kl[2w+1]) of the pair list with              */
/* wedge_ratio[w] = b_l / b_k.  "adjacency", "triplets", "component", "chordal" and "IRLS" run exactly as above; the     */
/* same handle type comes back.  tests/pairscales_np.py restates every point.  The host takes the logarithms and the     */
/* exponentials; on the device f64, unfused, only + - * / sqrt.                                                          */
/*   scale graph nodes = the translation pairs of the unscaled call; edges = the wedges with both ends among them and a  */
/*               finite ratio > 0 ("used").  Connected components by the kernels of csrc/graph_device.h; the one with    */
/*               the most pairs wins, the one with the smallest pair on a tie.  From here on the translation pairs       */
/*               (used_t, n_translation_pairs) are the pairs of that component, in_component the views they name (they   */
/*               are connected, since the two pairs of a wedge share a view), root its smallest view, C_root = 0; the rotations keep   */
/*               the gauge of "component" (R = I at its root), and R, C of a view outside are zero.  The view component  */
/*               may be smaller than the unscaled call's: reported (n_scaled_views), not an error.  No used wedge:       */
/*               every in_component is 0, the reports are filled, no error.                                               */
/*   scales      y_w = log(ratio_w).  Minimise sum rho(x_l - x_k - y) over the used wedges of the component, Huber in    */
/*               |x_l - x_k - y| with scale_delta (default 0.1), x of the component's smallest pair fixed at 0, from     */
/*               x = 0, by "IRLS" as for the rotations: per node sum_w w (dx_v - dx_n) = -+ w r (- in l's row, + in     */
/*               k's), by "PCG" with one value per node and preconditioner 1 / sum w, over a CSR adjacency of the scale  */
/*               graph (a node's wedges ascending by neighbour pair, built on the host; nodes of more than 64 wedges     */
/*               are gathered by a wave); x <- x + dx; the step rule and the stop codes of "IRLS".  Then b = exp(x)      */
/*               divided by the lower median of exp(x) over the translation pairs (element (n - 1) / 2 of n, sorted);    */
/*               b of every other pair is 0.                                                                              */
/*   centres     "translation" with r = (C_j - C_i) - b_k d_k and W = w I: Huber with translation_delta, whose default   */
/*               keeps its meaning as the median baseline is 1; the same Levenberg-Marquardt loop and PCG.               */
/* Known limit: a pair with no used wedge in the winning component drops out of the translation stage, and with it a     */
/* view that only such pairs reach.                                                                                       */
/* Refusals: those of sfmloc_global_poses; a wedge index out of range, k >= l, the same (k, l) twice, a wedge whose two   */
/* pairs share no view, scale_delta or a tolerance out of range: SFMLOC_EINVAL, before any launch.                        */
/* (The accessors are named sfmloc_gpscale_*: the handle is a sfmloc_gposes, and its sfmloc_gposes_* accessors serve it   */
/* unchanged.)                                                                                                            */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_gpscale_options {
  double   scale_delta;         /* Huber delta on the log ratio, default 0.1 */
  double   function_tolerance;  /* default 1e-6 */
  double   pcg_tolerance;       /* default 1e-6 */
  uint32_t max_steps;           /* default 50 */
  uint32_t max_pcg;             /* default 20000 iterations per solve */
} sfmloc_gpscale_options;
typedef struct sfmloc_gpscale_report {
  uint32_t n_wedges, n_wedges_used;      /* given; edges of the scale graph */
  uint32_t n_scaled_pairs, n_scaled_views; /* the winning component: its pairs, the views they name */
  uint32_t first_pair;                   /* its smallest pair, x = 0 */
  uint32_t steps_tried, steps_accepted, pcg_total, stop;   /* as rot_* of sfmloc_gposes_report */
  uint32_t launches;                     /* of the scale phase; sfmloc_gposes_report::launches counts the whole call */
  double   cost_initial, cost_final;     /* the robust cost at x = 0 and at the result */
  double   scale_ms;                     /* device time of the scale graph and the scale averaging */
  double   centre_ms;                    /* = sfmloc_gposes_report::translation_ms */
} sfmloc_gpscale_report;
void sfmloc_gpscale_default_options(sfmloc_gpscale_options *o);
/* opt, sopt NULL = the defaults */
int  sfmloc_global_poses_scaled(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs,
                                const double *rel_R /*[n_pairs*9]*/, const double *rel_t /*[n_pairs*3]*/,
                                const uint8_t *use_t /*[n_pairs], NULL = all*/, const sfmloc_gposes_options *opt,
                                const uint32_t *wedge_kl /*[n_wedges*2]*/, const double *wedge_ratio /*[n_wedges]*/,
                                uint32_t n_wedges, const sfmloc_gpscale_options *sopt, sfmloc_gposes **out);
/* b [n_pairs]: the baselines, 0 outside the translation pairs; all 0 on a handle of sfmloc_global_poses */
int  sfmloc_gpscale_baselines(const sfmloc_gposes *g, double *b /*[n_pairs]*/);
/* w [n_wedges]: the Huber weight of every wedge at the result, 0 for a wedge that is not used or outside the component */
int  sfmloc_gpscale_weights(const sfmloc_gposes *g, double *w /*[n_wedges]*/);
int  sfmloc_gpscale_report_read(const sfmloc_gposes *g, sfmloc_gpscale_report *rep);

/* ------------------------------------------------------------------------- */
/* Colouring plan of a map's landmarks (ColorizeTracks of openMVG_main_ComputeSfM_DataColor, the program the          */
/* reference runs after every reconstruction and merge): which view each landmark takes its colour from.  The greedy  */
/* cover runs on the structure exactly as sfmloc_sfm_create received it (the keep masks of sfmloc_sfm_clean and the   */
/* poses play no part); the host then reads the images in plan order and samples (sfmlocalization_amd/colorize.py,    */
/* csrc/colorize_cli.cpp).  OpenMVG 1.1 points are unpinned readings; each says which reading was chosen:             */
/*   counts      card[v] = the observations in view v of landmarks not coloured yet (every remaining landmark adds one */
/*               per observation, as the reference's recount does).  A landmark names a view once in the reference    */
/*               (Observations is a std::map); here one that names it twice counts twice.                             */
/*   choice      the view with the largest card; among equals the lowest view index (divergence: the reference sorts  */
/*               the counts with an unstable std::sort and takes the first, so its pick among equals is unspecified). */
/*   colouring   the chosen view colours every uncoloured landmark it observes, at that observation (the first one    */
/*               in CSR order when the landmark names the view twice).                                                */
/*   stop        when the largest card is 0.  A view without uncoloured observations is never chosen.  (Divergence:   */
/*               a landmark without observations makes the reference index an empty vector; here it stays uncoloured  */
/*               and the tools write it black.)                                                                       */
/*   arithmetic  integers only.  In one iteration a landmark is claimed by one lane only, and the decrements of card  */
/*               are atomicSub on uint32_t, the same result in any order: two runs give the same arrays.              */
/* The host enqueues SFMLOC_COLOR_CHUNK iterations at a time and reads the remaining-landmark count once per chunk;   */
/* launches queued behind the last iteration return at once.                                                          */
/* ------------------------------------------------------------------------- */
#define SFMLOC_COLOR_CHUNK 64u
/* order[k]   = view index chosen in iteration k, k < *n_order (n_order <= n_views; order holds n_views entries)
 * lm_iter[l] = iteration in which landmark l was coloured (every landmark with at least one observation gets one;
 *              0xFFFFFFFF for a landmark without observations)
 * lm_obs[l]  = index into obs_view / obs_x of the observation the colour is read at (0 for an uncoloured landmark)
 * lm_iter and lm_obs hold n_landmarks entries and may be NULL when there are none. */
int sfmloc_sfm_color_plan(sfmloc_sfm *h, uint32_t *order, uint32_t *n_order, uint32_t *lm_iter, uint64_t *lm_obs);
/* device milliseconds of the calling thread's last sfmloc_sfm_color_plan (HIP events around its kernels) */
double sfmloc_sfm_color_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Merging two maps (hulo_sfm/mergeSfM.py: mergeModel's RANSAC over 3D-3D matches, findMedianThres /                  */
/* findMedianStructurePointsThres, merge_sfm_data / transform_sfm_data), the step between the localiser and           */
/* OpenMVG_BA in the reference's mergeOneModel.  Points are host arrays [n*3]; A = model A's landmark, B = model B's, */
/* a match's model is M (3 x 4, row major) with A ~ M [B; 1].  Every solver uses + - * / sqrt in f64 only, unfused,   */
/* with fixed iteration counts, so tests/merge_np.py reproduces the bits.  Readings chosen and divergences:           */
/*   sampling    round r draws 4 distinct matches with ac_sample<4> (OpenMVG UniformSample over Philox4x32-10,        */
/*               key = params.seed, stage 3, the caller's stream, iteration r).  The reference uses Python's unseeded */
/*               random.sample: which rounds are drawn differs, the rule for the winner does not.                     */
/*   inlier      sqrt((dx dx + dy dy) + dz dz) < thres with d_i = (((m_i0 x0 + m_i1 x1) + m_i2 x2) + m_i3) - a_i.     */
/*               A match with a non-finite coordinate (mergeSfM.get3DPointloc: inf for a missing id) is never an      */
/*               inlier, and a sample that contains one counts nothing.                                               */
/*   winner      the round with the most inliers among those that pass the ratio test and have a finite model and at  */
/*               least one inlier; on ties the lowest round (the reference's sequential loop with its strict ">").    */
/*               Rounds are reduced with one integer maximum of (count << 32 | 0xFFFFFFFF - round): no float atomics, */
/*               the result does not depend on the launch geometry (params.rounds_per_launch).                        */
/*   jacobi      eigen-decompositions are cyclic Jacobi, 10 sweeps over (p, q) in row order, theta = (a_qq - a_pp) /  */
/*               (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta theta + 1)) (sign(0) = +1), c = 1 / sqrt(t t + 1), */
/*               s = t c; columns, then rows, then a_pq = a_qp = 0; a zero a_pq skips its rotation.                   */
/*   similarity  (model 0, build-defined reading: the reference imports Gohlke's transformations.py, whose text is    */
/*               not in its tree) both sets centred on their means (sum / count), S_ij = sum b0_i a0_j, the rotation  */
/*               maximising trace(R^T sum a0 b0^T) over proper rotations as Horn's unit quaternion: the eigenvector   */
/*               of the largest eigenvalue (first on ties) of the 4 x 4 matrix N(S), normalised; scale =              */
/*               sqrt(sum |a0|^2 / sum |b0|^2) (Gohlke's, not Umeyama's); t = mean(a) - s R mean(b).  The ratio of    */
/*               singular values of s R is 1 by construction: a finite model passes the ratio test.                   */
/*   affine      (model 1, mergeSfM.ransacAffineTransform) 4 points: [B; 1]^T X = A^T by Gaussian elimination with    */
/*               partial pivoting (in column k the rows below are compared with row k in order and swapped when       */
/*               strictly larger in magnitude), M = X^T.  The ratio test takes the singular values of M[:, :3] as     */
/*               square roots of the eigenvalues of L^T L (jacobi): sqrt(max) / sqrt(min) < svd_ratio.                */
/*   zero pivot  (divergence) a zero pivot makes the round count nothing, and makes the final fit fail (has_model 0): */
/*               numpy.linalg.lstsq returns the minimum-norm answer on such degenerate (coplanar) samples instead.    */
/*   final fit   on the winner's inliers (at least 4, else no model), ascending index: every sum is 256 partial sums  */
/*               (partial t adds elements t, t + 256, ... in order, from 0.0) joined by a pairwise tree (t += t + 128,*/
/*               then 64, ... 1).  Similarity: the means first, then the centred moments.  Affine: the 4 x 4 normal  */
/*               equations ([B; 1][B; 1]^T) X = [B; 1] A^T through the same elimination (lstsq uses an SVD; the two   */
/*               agree to rounding on well-conditioned sets).  The 4-point fits add their four terms in order.        */
/*   median      nearest other point: min over j != i of (dx dx + dy dy) + dz dz, one square root of the minimum      */
/*               (a duplicate at another index gives 0); the exact median of the n distances by a radix select on     */
/*               their bit patterns, (lo + hi) / 2 for even n; 0 for n < 2; non-finite coordinates: SFMLOC_EINVAL.    */
/*   transform   R' = M[:, :3] R, r'_ij = (m_i0 r_0j + m_i1 r_1j) + m_i2 r_2j (for a similarity that is s R: the      */
/*               reference's quirk, kept); X' = ((m_i0 x0 + m_i1 x1) + m_i2 x2) + m_i3.                               */
/*   caps        n > 2^24 or rounds >= 2^32: SFMLOC_ECAP, checked before anything else is touched.  n < 4: status 0, */
/*               no model.                                                                                             */
/* ------------------------------------------------------------------------- */
enum { SFMLOC_MERGE_SIMILARITY = 0, SFMLOC_MERGE_AFFINE = 1 };

typedef struct sfmloc_merge_params {
  uint64_t seed;              /* sampling key, as sfmloc_params.seed (same default) */
  int device;                 /* HIP device ordinal */
  uint32_t rounds_per_launch; /* RANSAC rounds per kernel launch; 0 = the library's choice.  Same result either way */
  int profile;                /* 1 = HIP events around the call's kernels: sfmloc_merge_last_ms */
  int reserved;
} sfmloc_merge_params;

typedef struct sfmloc_merge_result {
  double M[12];       /* the final fit on the winner's inliers; zeros when has_model = 0 */
  uint32_t has_model; /* 1 = a round won, it has at least 4 inliers and the final fit is finite */
  uint32_t round;     /* the winning round and its count (0, 0 when no round counted anything) */
  uint32_t count;
  uint32_t n_inliers; /* = count: the winner's inliers, listed in ascending index */
} sfmloc_merge_result;

void sfmloc_merge_default_params(sfmloc_merge_params *p);
/* ransacTransform (mergeSfM.py:344-399) with `rounds` rounds (the callers pass n * ransacRoundMul).  inliers may be
 * NULL; otherwise cap entries (SFMLOC_ECAP when the list is longer).  params may be NULL (the defaults). */
int sfmloc_merge_ransac(const double *A, const double *B, uint64_t n, double thres, uint64_t rounds, double svd_ratio,
                        int model, uint32_t stream, const sfmloc_merge_params *params, sfmloc_merge_result *out,
                        uint32_t *inliers, uint32_t cap);
/* getInliersByAffineTransform (mergeSfM.py:405-416): ascending indices of the matches within thres of M */
int sfmloc_merge_inliers(const double *A, const double *B, uint64_t n, const double *M /*[12]*/, double thres,
                         const sfmloc_merge_params *params, uint32_t *idx, uint32_t cap, uint32_t *n_out);
/* the median of every point's distance to its nearest other point (findMedianThres / ...StructurePointsThres / k) */
int sfmloc_merge_median_nn(const double *X, uint64_t n, const sfmloc_merge_params *params, double *median);
/* M applied in place to nR rotations [nR*9] and nX points [nX*3] (merge_sfm_data, transform_sfm_data) */
int sfmloc_merge_transform(const double *M /*[12]*/, double *R, uint64_t nR, double *X, uint64_t nX,
                           const sfmloc_merge_params *params);
/* device milliseconds between the events of the calling thread's last sfmloc_merge_* call made with profile = 1 */
double sfmloc_merge_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Thinning a map fixed to world coordinates (PyEvaluateAccuracy/src/localizeGlobalCoordinateRefPoint.py:81-118,      */
/* reduceClosePointsKDTree(sfmData, Amat, thres, knn), which --reduce-points runs with thres 0.01 and knn 1000):       */
/* landmarks closer than thres in world coordinates are folded into the one of lowest index.  Points are a host array */
/* [n*3] in structure order; the host appends observation lists in `order`.  f64, unfused, one expression per value, */
/* so tests/globalcoord_np.py reproduces the bits over an all-pairs matrix.  Readings chosen and divergences:         */
/*   global      G_i = ((a_i0 x0 + a_i1 x1) + a_i2 x2) + a_i3 (the "transform" arithmetic of sfmloc_merge); A = NULL  */
/*               is the identity through the same expression.                                                         */
/*   distance    d(i, j) = sqrt((dx dx + dy dy) + dz dz) on G (NumPy's norm may differ in the last bit).              */
/*   neighbours  N(i) = the min(knn, n) points nearest to i, i itself included, in ascending (d, index).  cKDTree's   */
/*               order among equal distances is unspecified: this reading is build-defined.                           */
/*   close set   C(i) = { j in N(i) : j > i and d(i, j) < thres }: only the lower index's list counts, as there.      */
/*   greedy      in ascending i an unabsorbed i is a keeper and absorbs every j of C(i) that is still unabsorbed, in  */
/*               N(i)'s order; that is: i is a keeper iff no keeper k < i has i in C(k), and an absorbed j belongs to */
/*               the smallest such keeper.  Not transitive: d(0,1) < thres, d(1,2) < thres, d(0,2) >= thres absorbs 1 */
/*               and keeps 2.  (The reference's brute-force reduceClosePoints agrees wherever knn does not bind.)      */
/*   outputs     owner[i] = i for a keeper, else its keeper; dist[i] = d(owner[i], i), 0 for a keeper; order = the    */
/*               absorbed points grouped by ascending owner, inside a group by (dist, index): the order in which the  */
/*               reference appends their observations; the other n - n_absorbed entries are 0xFFFFFFFF.  n_pairs =    */
/*               the sum of |C(i)|; rounds = the passes of the greedy resolution (a point is decided in the pass      */
/*               after the last of the points that list it; 1 when no point lists another).  None of it depends on    */
/*               params.rounds_per_launch (here: resolution passes between two host checks; 0 = the library's).       */
/*   method      a uniform grid of cell thres (1 + 2^-10) over the bounding box of G, hashed; points within thres are */
/*               always the nearest ones, so nothing outside a point's 27 cells is needed.                            */
/*   n < 2       (divergence) nothing is absorbed, rounds 0; the reference's query fails on k = 1.                     */
/*   refusals    non-finite A, X or thres, thres <= 0: SFMLOC_EINVAL.  n > 2^24, more than 2^21 cells on an axis      */
/*               (which includes a world coordinate that overflows), more than 2^28 close pairs: SFMLOC_ECAP.  Every  */
/*               check happens before owner, order, dist or *out is written.                                          */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_reduce_result {
  uint64_t n_keep, n_absorbed, n_pairs;
  uint32_t rounds, reserved;
} sfmloc_reduce_result;
int sfmloc_reduce_points(const double *X /*[n*3]*/, uint64_t n, const double *A /*[12] or NULL = identity*/, double thres,
                         uint32_t knn, const sfmloc_merge_params *params, uint32_t *owner /*[n]*/, uint32_t *order /*[n]*/,
                         double *dist /*[n]*/, sfmloc_reduce_result *out);
/* device milliseconds between the events of the calling thread's last sfmloc_reduce_points made with profile = 1 */
double sfmloc_reduce_last_ms(void);

/* ------------------------------------------------------------------------- */
/* All-views BoW k-NN (the pair list of a map under construction: for every view the k views nearest to it in BoW     */
/* space, which sfmlocalization_amd.bowpairs / ComputeBoWPairs turn into the pair file ExtFeatAndMatch -p reads).  Row */
/* i is what sfmloc_bow_select answers for the query bow[i] over the candidates cand(i); the call takes no handle and  */
/* works on host arrays, bow [n * dim] float32 row-major.                                                              */
/*   distance    d(i, j) = the float32 squared L2 distance of sfmloc_bow_select (oracle/sfm_oracle_bow.c orc_bow_dist): */
/*               64 partial sums, partial l adds (a - b) * (a - b) for the elements l, l + 64, ... in index order,      */
/*               unfused; then partial[l] + partial[l ^ stride] for the strides 32, 16, 8, 4, 2, 1.  d(i, j) and        */
/*               d(j, i) have equal bits.                                                                              */
/*   candidates  cand(i) = { j : |j - i| > window }: window = 0 leaves out only i itself; a caller that already pairs  */
/*               every view with its `window` neighbours in sequence spends k on the other views.                      */
/*               count[i] = min(k, |cand(i)|).                                                                          */
/*   selection   the count[i] candidates smallest in (distance bits, index): ties go to the lower index.  nbr[i*k ..]  */
/*               holds them in ASCENDING INDEX (as sfmloc_bow_select returns a shortlist), dist[i*k + s] the distance  */
/*               of nbr[i*k + s]; the slots from count[i] on hold 0xFFFFFFFF and +inf.                                  */
/*   +inf        a distance that overflows to +inf from finite vectors is a distance like any other: above every       */
/*               finite one, below an entry that is no candidate.                                                       */
/*   nothing     n < 2 or window >= n - 1: every count is 0, every slot padding, SFMLOC_OK, nothing is launched.        */
/*   refusals    all before anything is allocated or launched (they come back on a machine without a GPU), no output   */
/*               written: k = 0, dim = 0, a NULL array with n > 0, a NaN or infinite entry of bow ("row 3 has a         */
/*               non-finite value"): SFMLOC_EINVAL.  n > 2^22, n * k > 2^32 entries: SFMLOC_ECAP.                        */
/*   memory      the n x n distances never exist at once: a pass computes the distances of rows_per_launch query rows   */
/*               to all n views into a scratch of rows_per_launch * n uint32 and selects from it, then the next pass.   */
/*               rows_per_launch = 0: the library's, 2^26 / n rows rounded down to a multiple of 16 (at least 1, at     */
/*               most n): a scratch of at most 256 MB, two passes at n = 10 000.  Beside it: bow itself and the         */
/*               results of one pass.  No bit of any output depends on rows_per_launch.                                 */
/*   profile     1: sfmloc_bowknn_last_ms is the device time between two events around the passes (the kernels and the */
/*               copies of each pass's results to the host); 0 otherwise.                                               */
/* FLANN's approximate KD-tree search of the reference (BoFUtils.cpp:46-59) is replaced by the exact search, as in       */
/* sfmloc_bow_select.                                                                                                    */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_bowknn_options {
  uint32_t k;                /* neighbours per view, >= 1 */
  uint32_t window;           /* candidates of row i: every j with |j - i| > window; 0 excludes only i itself */
  uint32_t rows_per_launch;  /* query rows per distance/select pass; 0 = the library's; no output depends on it */
  uint32_t profile;          /* 1: time the call between two events */
} sfmloc_bowknn_options;
void   sfmloc_bowknn_default_options(sfmloc_bowknn_options *o);   /* k 20, window 0, 0, 0 */
/* opt NULL = the defaults */
int    sfmloc_bow_knn(int device, const float *bow /*[n*dim]*/, uint32_t n, uint32_t dim,
                      const sfmloc_bowknn_options *opt,
                      uint32_t *nbr /*[n*k]*/, float *dist /*[n*k]*/, uint32_t *count /*[n]*/);
/* device milliseconds of the calling thread's last sfmloc_bow_knn made with profile = 1 */
double sfmloc_bowknn_last_ms(void);

/* ------------------------------------------------------------------------- */
/* Map-side matching: the reference's matchAKAZE /         */
/* trackAKAZE on the same kernels.  Views are addressed by their index in the  */
/* map's view table (ascending view id).                                       */
/* ------------------------------------------------------------------------- */
typedef struct sfmloc_matches sfmloc_matches; /* PairWiseMatches: std::map<Pair, vector<IndMatch>> flattened */

/* The descriptors (and keypoints) of one map image as a query object, rebuilt on the device from the bank: what
 * the reference obtains by re-reading <base>.desc for the second image of a pair (MatchUtils.cpp:85-96). */
int sfmloc_query_from_view(sfmloc_map *map, uint32_t view_index, sfmloc_query **out);

/* matchAKAZE's per-pair body (MatchUtils.cpp:99-150) for first = each selected view, second = the query:
 * 2-NN + ratio of every row of `first` among the query's rows (sfmloc_match_putative), then the one-to-one filter
 * (a query row hit twice or more loses all its hits, :125-143) and the emit loop that never emits the last row of
 * `first` (:146).  Results are read with sfmloc_putative_read. */
int sfmloc_match_one_to_one(sfmloc_map *map, sfmloc_query *query, const uint32_t *view_sel, uint32_t n_sel);

/* hulo::matchAKAZE (MatchUtils.cpp:73-152): pairs[2k], pairs[2k+1] = (first, second) view indices; images with
 * fewer than 2 descriptors are skipped (:101-103); pairs without matches get no entry. */
int sfmloc_match_pairs(sfmloc_map *map, const uint32_t *pairs, uint32_t n_pairs, sfmloc_matches **out);

/* hulo::trackAKAZE (MatchUtils.cpp:156-277) over the map's views in table order: consecutive-frame matches as
 * above, then chained up to max_frame_dist frames apart (:240-276).  Every consecutive pair has an entry (possibly
 * empty), longer-range pairs only when non-empty, as the reference's std::map ends up. */
int sfmloc_track(sfmloc_map *map, uint32_t max_frame_dist, sfmloc_matches **out);

/* hulo::geometricMatch (MatchUtils.cpp:372-420) for map image pairs: F-matrix AC-RANSAC (params.ransac_round,
 * params.geom_precision) on the given putative lists -- pair k = (pairs[2k], pairs[2k+1]) owns
 * match_i/j[offsets[k] .. offsets[k+1]) -- keeping a pair iff it has more than 2.5*7 inliers; the surviving matches
 * come in AC-RANSAC's inlier order.  No minimum list length is applied here (the caller applies ExtFeatAndMatch's
 * minMatch, computeFeaturesAndMatches.cpp:211-221).  With params.guided_matching a surviving pair's matches are
 * replaced by the guided ones (all features of both images under the estimated F, one per feature of I, ascending;
 * possibly none -- the pair keeps its entry, as in Robust_model_estimation). */
int sfmloc_geometric_pairs(sfmloc_map *map, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                           const uint32_t *match_i, const uint32_t *match_j, sfmloc_matches **out);

uint32_t sfmloc_matches_pairs(const sfmloc_matches *m); /* number of (I, J) entries, ascending (I, J) */
int sfmloc_matches_pair(const sfmloc_matches *m, uint32_t k, uint32_t *view_i, uint32_t *view_j, uint32_t *n);
int sfmloc_matches_read(const sfmloc_matches *m, uint32_t k, uint32_t *i, uint32_t *j, uint32_t cap);
void sfmloc_matches_destroy(sfmloc_matches *m);

/* Parity probe: runs one of the f64 device building blocks over n items (tests compare with the oracle).
 * op: 0 log10, 1 sqrt+div, 2 cubic, 3 quartic, 4 seven-point, 5 P3P, 6 KRt_From_P, 7 sample,
 *     8 seven-point, wave-parallel form (K3's fast kernel; layout of op 4), 11 six-point resection (below) */
int sfmloc_debug_math(int device, int op, const double *in, int n, int in_stride, double *out, int out_stride);
/* ------------------------------------------------------------------------- */
/* Uncalibrated queries: the six-point resection ("resect6").                  */
/* RESTATED, UNVERIFIED AGAINST OpenMVG: the library's sources were not at     */
/* hand.  This section is what the code computes; tests/resect6_np.py restates */
/* every operation in NumPy and the GPU tests compare bits with it.            */
/*                                                                             */
/* sfm::SfM_Localizer::Localize without an intrinsic: AC-RANSAC over           */
/* ACKernelAdaptorResection<SixPointResectionSolver, ...>, then KRt_From_P on  */
/* the winning projection matrix.  For a query marked with                     */
/* sfmloc_query_set_uncalibrated, sfmloc_match_set, sfmloc_resection,          */
/* sfmloc_localize, sfmloc_localize_bow, sfmloc_localize[_bow]_begin / _end    */
/* and sfmloc_localize_batch do this instead of P3P.  Readings chosen:         */
/*   2D points   the query's raw feature pixels: get_ud_pixel is not applied,  */
/*               nothing of the map's intrinsic is used.                       */
/*   N1          NormalizePoints in the (width, height) form: x' = (x - w/2)   */
/*               / sqrt(w h), y' = (y - h/2) / sqrt(w h), computed as          */
/*               x * (1/f) + (-(w/2) * (1/f)) with f = sqrt(w h) -- the same   */
/*               expression the calibrated path evaluates with K.              */
/*   sample      six distinct correspondences, one model: the counter-based    */
/*               sampler of K5 (Philox4x32-10 keyed by params.seed, counter    */
/*               {iteration, stream 0, draw / 4, stage 4}), sorted positions.  */
/*   design      the 3D points are translated so that the first sampled one is */
/*               the origin (X' = X - X0); two rows per point,                 */
/*                 [X' Y' Z' 1  0 0 0 0  -xX' -xY' -xZ' -x]                     */
/*                 [0 0 0 0  X' Y' Z' 1  -yX' -yY' -yZ' -y],  12 x 12.          */
/*   null vector G = D^T D (every entry the sum over the 12 rows in row order, */
/*               zeros included), then cyclic Jacobi on G: 10 sweeps over      */
/*               (p, q) in row order, the rotation of `jacobi` in the          */
/*               sfmloc_merge section, a zero g_pq skipped.  The model is the  */
/*               column of V of the smallest diagonal entry (the first on      */
/*               ties), row major 3 x 4, then P = P' [I | -X0].                */
/*   rank        no model for the sample when the second smallest diagonal     */
/*               entry is <= 1e-12 x the largest (coplanar or repeated points: */
/*               the null space is not a line) or an entry of P is not finite. */
/*   sign        P is negated when more than three of the six sampled points   */
/*               have negative depth p3 . (X, 1).                              */
/*   residual    squared reprojection error against the normalised points;     */
/*               logalpha0 = log10(pi); NFA with MAX_MODELS 1, sample size 6.  */
/*   AC-RANSAC   K5's: params.p3p_max_iteration, the 10 % reserve and the      */
/*               early-iteration reduction, residual order (error, index).     */
/*   refinement  params.refine_pose = 1: after KRt_From_P, R and t are refined  */
/*               on the inliers' raw pixels (the calibrated path's Levenberg-  */
/*               Marquardt, at most 20 steps) under the recovered K -- fx,     */
/*               skew, cx, fy, cy -- held fixed; pose.K stays the recovered    */
/*               one and pose.P = K [R|t] of the refined pose.                 */
/*   afterwards  P = N1^-1 M; error_max = sqrt(e) * sqrt(w h) (pixels); more   */
/*               than 2.5 * 6 inliers, then params.min_inliers (">");          */
/*               KRt_From_P: pose.K is the RECOVERED intrinsic; center = -R^T  */
/*               t.  A query with <= max(min_resection_points, 6) 2D-3D        */
/*               matches is not localised (ok = 0, no error).                  */
/* Divergences / left out:                                                     */
/*   - the null vector comes from the fixed-sweep Jacobi of D^T D, not from an */
/*     SVD of D: the bits differ from Eigen's, the tie rule is this one's.     */
/*   - the rank rule and the majority form of the sign rule are this           */
/*     library's.                                                              */
/*   - the translation of the sample's 3D points to its first point before D   */
/*     is built, undone by P = P' [I | -X0], is this library's conditioning of */
/*     the 3D side; the sampled image points are NOT conditioned again per     */
/*     sample (N1 of the image is the only conditioning of the 2D side).       */
/*   - a scene in which no sample ever has a model ends with nfa = error_max = */
/*     +inf and a zero pose, as a calibrated query without a model does.       */
/*   - gang sessions (a marked query begun on a context inside                 */
/*     sfmloc_gang_begin / _end) and the sharded entry points                  */
/*     (sfmloc_shard_begin, sfmloc_shard_bow_keys, sfmloc_shard_begin_bow,     */
/*     sfmloc_merge_begin[_packed] and their _batch forms): SFMLOC_EINVAL for  */
/*     a marked query; sfmloc_last_error says so.                              */
/* An unmarked query's result is bit for bit what it was.                      */
/* ------------------------------------------------------------------------- */
/* Parity probe of the whole stage: the six-point AC-RANSAC on the given n 2D-3D correspondences (pixels, world) of an
 * image of width x height, on the map's own context with the map's params; the inliers' indices (AC-RANSAC's order)
 * into inlier_idx when the pose is ok.  sfmloc_debug_math op 11 is the solver alone: a row of x[12] (six image points)
 * and X[18] in, the model count (0 / 1) and the 12 model entries out. */
int sfmloc_debug_resect6(sfmloc_map *map, const double *pt2d, const double *pt3d, uint32_t n, uint32_t width,
                         uint32_t height, sfmloc_pose *out, uint32_t *inlier_idx, uint32_t cap);
/* Test hook: allocation k (0..11) of the NEXT regrowth of a context's P3P workspace fails with SFMLOC_ENOMEM (one shot;
 * -1 disarms).  The regrowth has no counterpart in the reference (localization.cpp:479-509 has no size limit). */
void sfmloc_debug_fail_p3p_alloc(int k);
/* Test hook: the calling thread's k-th device allocation from now on (0 = the next) fails once with SFMLOC_ENOMEM, in
 * whatever call makes it; -1 disarms.  An armed sfmloc_debug_fail_p3p_alloc takes the countdown over for its regrowth. */
void sfmloc_debug_fail_next_alloc(int k);
/* The geometric filter's register forms keep, per wave, the sorted match list of the model the wave evaluated last.
 * out[0]: how often a view's new best model took its inlier list from there, out[1]: how often one wave had to evaluate
 * the model again for it, on `device`, by every map of the process since the last reset (reset != 0 clears both after
 * reading; out may be null).  Synchronises the device.  For tests: the two ways give the same list. */
int sfmloc_debug_k3_list_counts(int device, uint64_t *out, int reset);
/* The launch forms the P3P AC-RANSAC rounds were queued in, by every context of the process since the last reset:
 * out[0] small rounds (k_p3p_round_small), out[1] plain rounds (k_p3p_round, one workgroup per hypothesis), out[2] wide
 * rounds (k_p3p_round, one workgroup per model).  Counted on the host where a round is queued, inside a gang session or
 * not -- a round that finds the stage finished, or a small round that leaves a larger set to the full form, counts all
 * the same; six-point rounds are not counted.  reset != 0 clears the three after reading; out may be null.
 * Synchronises the device.  For tests: every form gives the same bits, so nothing else shows which one ran. */
int sfmloc_debug_k5_round_counts(int device, uint64_t *out, int reset);
/* The view list the context's last begin (sfmloc_localize[_bow]_begin, sfmloc_shard_begin[_bow], inside a finished gang
 * session or not) worked on, read back after synchronising the context's stream: *n entries into views -- ascending view
 * indices; a sharded shortlist's padding appears as written, as the phantom index n_views; every view in order when the
 * begin took all views.  SFMLOC_ECAP, with *n set, when cap < *n.  For tests: the selection a shortlist built on the
 * device never reaches the host otherwise. */
int sfmloc_debug_context_views(sfmloc_context *ctx, uint32_t *views, uint32_t cap, uint32_t *n);

/* ------------------------------------------------------------------------- */
/* Measurement (params.profile = 1): accumulated HIP-event time per kernel on  */
/* the handle's stream.                                                        */
/* ------------------------------------------------------------------------- */
enum {
  SFMLOC_K_HAMMING = 0,
  SFMLOC_K_COMPACT = 1,
  SFMLOC_K_FMATRIX = 2,
  SFMLOC_K_MATCHSET = 3,
  SFMLOC_K_P3P = 4,
  SFMLOC_K_BOW = 5,
  SFMLOC_K_COUNT = 8
};
typedef struct sfmloc_kernel_stats {
  double total_ms[SFMLOC_K_COUNT];
  uint64_t launches[SFMLOC_K_COUNT];
  uint64_t hamming_pairs;      /* bank rows x query rows compared since reset */
  uint64_t hamming_alg_bytes;  /* 64*rows + 64*Nq + 12*matches is finalised by the caller */
  uint64_t hamming_lane_ops;       /* VALU lane-instructions K1 issued for those pairs (35 per exact pair; fewer when
                                      the screening kernel rejects a pair on its prefix distance).  For scans on the
                                      matrix cores (params.k1_mfma) it counts what that kernel issues on the VALU --
                                      operand expansion and the running maximum, 2.25 per pair -- the MFMA work itself
                                      is not in it */
  uint64_t hamming_pairs_finished; /* screened pairs whose full distance had to be computed (popcount form only: the
                                      matrix-core form computes every distance in full and counts none here) */
  uint64_t hamming_rows_flagged;   /* bank rows the screening kernel handed to the exact kernel */
} sfmloc_kernel_stats;
int sfmloc_stats_read(sfmloc_map *map, sfmloc_kernel_stats *out); /* synchronises */
int sfmloc_stats_reset(sfmloc_map *map);
/* Changes params.profile of a live map: 0 = no events, 1 = every stage bracketed, 2 = the Hamming scan only.  Each
 * bracketed stage costs two marker packets on the stream (about 10 us of idle GPU between dependent kernels), so a
 * latency measurement wants 0 or 2. */
int sfmloc_set_profile(sfmloc_map *map, int level);

#ifdef __cplusplus
}
#endif
#endif /* SFMLOC_H */
