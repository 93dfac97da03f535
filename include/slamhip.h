/* include/slamhip.h -- C-ABI of the MI355X (gfx950) scan-matching / particle-likelihood engine.
 *
 * Drop-in boundary for ONE hot path of OSLL/slam-constructor: the GridScanMatcher (MC/HC/BF)
 * accept loop and the ScanProbabilityEstimator scoring it calls for every candidate pose and
 * every GMapping particle, plus the particle weight/normalise/resample step.
 *
 * The reference has no FFI: the path sits behind C++ virtual interfaces in headers.  Each entry
 * point below names the reference interface (file:line, relative to the reference root) whose
 * work it replaces; INTEGRATION.md shows the adapter classes (deriving from the reference's
 * GridScanMatcher / ScanProbabilityEstimator) that bind them.
 *
 * Conventions: plain C, pointers + sizes, no C++/torch types.  Every function returns 0 on
 * success or a negative slamhip_status; slamhip_last_error() gives the text.  One context =
 * one GPU + one HIP stream + one caller thread (the reference is single-threaded:
 * src/ros/single_hypoth_slam_node.cpp:63); contexts are independent (one per GPU when
 * particles are sharded).  There is NO CPU fallback: without a usable GPU the calls fail.
 *
 * All arithmetic is IEEE double in the reference's operation order (built with
 * -ffp-contract=off); see DESIGN.md for the exact-parity contract.
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMHIP_VERSION 100

typedef enum {
  SLAMHIP_OK = 0,
  SLAMHIP_ERR_INVALID = -1,   /* bad argument / unknown id */
  SLAMHIP_ERR_HIP = -2,       /* HIP runtime error (text in slamhip_last_error) */
  SLAMHIP_ERR_NO_DEVICE = -3, /* no usable GPU: the product path never falls back to the CPU */
  SLAMHIP_ERR_STATE = -4,     /* call order (e.g. scoring before a scan/map was uploaded) */
  SLAMHIP_ERR_UNSUPPORTED = -5,
  SLAMHIP_ERR_TIMEOUT = -6    /* a collective of the shard group did not complete within the group's deadline */
} slamhip_status;

/* Cell payload models mirrored in HBM:
 *  OCC      1 x f64  prob_occ            GridCell / MeanProbabilityCell / AffineQualityMergeCell
 *                                        (src/core/maps/grid_cell.h:33-35, naive_grid_cells.h:6-44)
 *  TBM      4 x f64  (u, e, o, c)        TbmBaseCell belief (src/core/maps/tbm_grid_cells.h:21-35)
 *  GMAPPING 3 x f64  (prob_occ, obst.x, obst.y)  GmappingBaseCell
 *                                        (src/slams/gmapping/gmapping_grid_cell.h:9-43)
 *  CREDIBILIST 4 x f64 (u, e, o, c)     CredibilistCell belief (src/slams/credibilist/grid_cell.h:10-68): the TBM
 *                                        payload, host stride and unknown_payload, updated by SLAMHIP_RULE_TBM
 *                                        (its operator+= is TbmBaseCell's, operation for operation), but SCORED by
 *                                        its own rule: discrepancy = 1 - disjunctive(observation, belief).occupied()
 *                                        (grid_cell.h:31-40, transferable_belief_model.h:145-162).  Like TBM it takes
 *                                        the discrepancy OIE only and never the GMapping OOPE. */
enum { SLAMHIP_CELL_OCC = 0, SLAMHIP_CELL_TBM = 1, SLAMHIP_CELL_GMAPPING = 2, SLAMHIP_CELL_CREDIBILIST = 3 };
/* OccupancyObservationProbabilityEstimator kinds
 * (src/core/scan_matchers/occupancy_observation_probability.h:12-99,
 *  src/slams/gmapping/gmapping_occupancy_observation_pe.h:11-45) */
enum { SLAMHIP_OOPE_OBSTACLE = 0, SLAMHIP_OOPE_MAX = 1, SLAMHIP_OOPE_MEAN = 2,
       SLAMHIP_OOPE_OVERLAP = 3, SLAMHIP_OOPE_GMAPPING = 4 };
/* ObservationImpactEstimator kinds (src/core/scan_matchers/observation_impact_estimators.h:14-28) */
enum { SLAMHIP_OIE_DISCREPANCY = 0, SLAMHIP_OIE_OCCUPANCY = 1 };
/* Per-pose summation order of sum_i p_i*w_i*factor_i (weighted_mean_point_probability_spe.h:124):
 *  TREE256    canonical, launch-shape independent tree (default; ~1e-16 from the reference)
 *  SEQUENTIAL the reference's beam-order sum, bit-exact (slower: second pass) */
enum { SLAMHIP_SUM_TREE256 = 0, SLAMHIP_SUM_SEQUENTIAL = 1 };
/* Where sin/cos of the pose heading come from (TrigonometryProvider::set_base_angle,
 * src/core/trigonometry_utils.h:31-33,57-60): host libm (bit-exact with the reference) or the
 * device's sincos (default for throughput; differs from glibc in the last ulp at most). */
enum { SLAMHIP_POSE_TRIG_DEVICE = 0, SLAMHIP_POSE_TRIG_HOST = 1,
       /* RAW_EXACT: the reference's DEFAULT provider bit for bit -- RawTrigonometryProvider evaluates std::cos / std::sin
        * (theta + a) per beam and pose (trigonometry_utils.h:17-35; use_trig_cache = false, src/ros/init_utils.h:56-58).
        * The device evaluates glibc 2.35's sin / cos restated operation for operation (csrc/libm_exact.h: the build of
        * them this host's libm runs, slamhip_libm_variant) on theta + a; needs the beam angles (slamhip_scan_set_angles
        * or slamhip_scan_filter_upload).  Host-driven and slow: the mode results are checked against, not a fast path. */
       SLAMHIP_POSE_TRIG_RAW_EXACT = 2 };
enum { SLAMHIP_TRIG_RAW = 0, SLAMHIP_TRIG_CACHED = 1 };

typedef struct slamhip_ctx slamhip_ctx;
typedef struct slamhip_matcher slamhip_matcher;

/* ScanProbabilityEstimator configuration = what init_spe/init_oope/init_oie build
 * (src/utils/init_scan_matching.h:27-113) + ScanProbabilityEstimator::SPEParams
 * (src/core/scan_matchers/grid_scan_matcher.h:87-91). */
typedef struct {
  int oope;              /* SLAMHIP_OOPE_* */
  int oie;               /* SLAMHIP_OIE_* */
  double area[4];        /* sp_analysis_area: bot, top, left, right (all 0 = point) */
  double gm_fullness_th; /* GmappingOccupancyObservationPE(fullness_th, window) */
  int gm_window;
  int sum_order;         /* SLAMHIP_SUM_* */
  int pose_trig;         /* SLAMHIP_POSE_TRIG_* */
} slamhip_spe_cfg;

/* ---------------------------------------------------------------- context */
const char *slamhip_last_error(void);
int slamhip_device_count(int *count);
int slamhip_ctx_create(int device, slamhip_ctx **out);
int slamhip_ctx_destroy(slamhip_ctx *ctx);
int slamhip_ctx_synchronize(slamhip_ctx *ctx);
/* hipStream_t of the context, for callers that enqueue their own work around ours */
void *slamhip_ctx_stream(slamhip_ctx *ctx);
/* Options of a context.  Every option switches between execution paths that give the SAME results (the parity tests
 * and the measurements in DESIGN.md run both sides); the library reads no environment variables.  Set them before the
 * objects they concern are created or used. */
enum {
  SLAMHIP_OPT_LOW_LATENCY = 0,   /* 1 (default): results come back through pinned completion words the host polls,
                                  * poses are read over PCIe by the kernels; 0: stream synchronisation */
  SLAMHIP_OPT_STAGE_POSES = 1,   /* 1: pose batches are copied to HBM before a scoring kernel reads them; 0 (default) */
  SLAMHIP_OPT_FILTER_CHAINS = 2, /* 1 (default): a filter step runs one accept chain per particle on the device;
                                  * 0: the host-driven lock-step jobs */
  SLAMHIP_OPT_K6_PATH = 3,       /* single-scan map update: 0 (default) the fastest pipeline that applies (gather,
                                  * else counting sort, else radix sort), 1 counting sort, 2 radix sort */
  SLAMHIP_OPT_K6_BATCH_FAST = 4, /* batched map update: 1 (default) free observations of zero-mean cells are settled
                                  * with atomics and only the rest is sorted; 0: every record is sorted into its chain */
  SLAMHIP_OPT_RESIDENT_CHAINS = 6, /* 1 (default): the filter's per-particle accept chains run as ONE launch of
                                    * co-resident workgroups when they all fit the device (csrc/hc_resident_gm.hip);
                                    * 0: a kernel per super-step (csrc/hc_chain.hip).  Same results either way. */
  SLAMHIP_OPT_K6_BATCH_KEY64 = 5, /* batched map update: 1 forces the 8-byte (particle, cell) keys of very large
                                   * batches; 0 (default): by size */
  SLAMHIP_OPT_TBM_PLANE = 7,     /* 1 (default): the 1-cell scorers over a TBM map gather the cell's per-beam
                                  * probability -- a pure function of the cell (tbm_grid_cells.h:21-35 with the fixed
                                  * observation of the scorer) -- from an 8-byte plane every writer of the map keeps,
                                  * instead of the 32-byte cell and its belief arithmetic per (pose, beam); 0: from the
                                  * cell.  The same operations either way: the same bits.  Governs
                                  * SLAMHIP_CELL_CREDIBILIST maps too (their plane holds that model's probability). */
  SLAMHIP_OPT_RAW_PROLOGUE = 9,  /* slamhip_matcher_process_raw_scan, a lone hill-climbing match that runs as ONE launch of
                                  * co-resident workgroups (1-cell OOPE, default sum order).  1 (default): the filtered scan
                                  * is not assembled in HBM by a kernel in front of the match; every workgroup of the
                                  * chain makes its beams' constants itself from the staged scan and the resident
                                  * per-beam tables, and the chain writes the scan block for whoever comes after it
                                  * (csrc/hc_resident.hip, RAW).  0: the assembly kernel, then the chain.  Every other
                                  * match is behind the assembly kernel either way.  The same bits in both. */
  SLAMHIP_OPT_RAW_PROLOGUE_MATCHES = 10, /* read-only (slamhip_ctx_get_option): matches of this context so far whose
                                          * chain assembled the scan itself and reported a result */
  SLAMHIP_OPT_INERT_TAIL = 8     /* the tail of a hill-climbing chain on the device (1-cell OOPE).  The reference's enumerator
                                  * stops at a count of failed rounds, not at convergence
                                  * (hill_climbing_scan_matcher.h:83-101), the steps halved at every failure.
                                  * 1: once the steps are below half an ulp of every pose coordinate, every candidate
                                  * of every further round IS the best pose, bit for bit: the same score, `best < score`
                                  * false (pose_enumeration_scan_matcher.h:58) -- the chain ends there; the remaining
                                  * 6 x (limit - failed rounds) + 1 scorer calls are reported to the observer and
                                  * counted, not scored again.  2 (default): also once a tree's walk has accepted
                                  * nothing and the steps have become so small that every beam of every further
                                  * candidate provably ends in the same cell as under the best pose (a per-beam bound
                                  * on the end point's movement against its distance from the cell's edges, made by the
                                  * chain's idle bookkeeping workgroup: csrc/hc_resident.hip "certificate"): the same
                                  * cells, the same terms, the same score (co-resident form only; the chain of kernels
                                  * stays at 1).
                                  * 0: every call scored.  Same traces, results and counts in all three. */
};
int slamhip_ctx_set_option(slamhip_ctx *ctx, int option, int value);
int slamhip_ctx_get_option(slamhip_ctx *ctx, int option, int *value);

/* ---------------------------------------------------------------- map mirror
 * Replaces GridMap::operator[] on the scoring path (src/core/maps/grid_map.h:62,
 * plain_grid_map.h:27-42,69-73, lazy_tiled_grid_map.h:47-55,140-147): the adapter mirrors the
 * cells into a dense pitched HBM window.  Coordinates are INTERNAL (external + origin,
 * regular_squares_grid.h:141-143); reads outside the window return `unknown_payload`, exactly
 * like Unbounded*GridMap::operator[] returns its prototype cell. */
int slamhip_map_bind(slamhip_ctx *ctx, int map_id, int cell_model, int width, int height,
                     int origin_x, int origin_y, double scale, const double *unknown_payload);
/* payload: host, row-major [h][w][stride]; window at internal (x0, y0) */
int slamhip_map_upload_window(slamhip_ctx *ctx, int map_id, int x0, int y0, int w, int h,
                              const double *payload);
/* GridMap::update / reset (src/core/maps/grid_map.h:41-60) forwarded as a dirty-cell log:
 * n cells, coords_xy internal (2 ints each), payloads n*stride doubles */
int slamhip_map_apply_dirty(slamhip_ctx *ctx, int map_id, int n, const int *coords_xy,
                            const double *payloads);
/* Unbounded maps move their origin when they grow (plain_grid_map.h:133-173): re-bind keeps
 * the old cells at their shifted place. */
int slamhip_map_release(slamhip_ctx *ctx, int map_id);
/* An UNBOUNDED map in HBM (UnboundedPlainGridMap, src/core/maps/plain_grid_map.h:52-176): with on = 1 a
 * slamhip_map_append_scan that reaches beyond the window grows it first -- a re-bind that keeps every cell at its
 * external coordinates, the new area holding the unknown payload -- instead of failing.  The reference grows
 * inside GridMap::update, cell by cell, by ensure_inside's Expansion_Rate rule (:133-173); the window here is a
 * superset of that one with the same cells.  This is what lets a single-hypothesis world keep its map on the GPU
 * (host/slamhip_resident_world.h). */
int slamhip_map_set_auto_grow(slamhip_ctx *ctx, int map_id, int on);
/* geometry of a bound window (RegularSquaresGrid::width/height/origin/scale, regular_squares_grid.h:26-38,141-143)
 * and how often it has grown; any out pointer may be NULL */
int slamhip_map_info(slamhip_ctx *ctx, int map_id, int *cell_model, int *width, int *height, int *origin_x,
                     int *origin_y, double *scale, long long *times_grown);
/* read back a window (tests / debugging) */
int slamhip_map_download_window(slamhip_ctx *ctx, int map_id, int x0, int y0, int w, int h,
                                double *payload_out);

/* ---------------------------------------------------------------- map render (csrc/map_render.hip)
 * A resident map as the bytes its consumers take, one byte per cell, converted ON THE DEVICE: a kernel reads the
 * cells (8 or 32 bytes each) and writes w * h bytes into a buffer the context owns, ONE asynchronous copy and one wait
 * bring them to `out` -- instead of the whole payload over PCIe and a conversion on the host.
 *   SLAMHIP_RENDER_OCCGRID  int8, rows bottom-up (y ascending): nav_msgs::OccupancyGrid::data as
 *                           OccupancyGridPublisher::on_map_update fills it (src/ros/occupancy_grid_publisher.h:37-46):
 *                           value == -1 ? -1 : (int)(value * 100).  The reference's conversion is undefined for a
 *                           value that is not finite: such a cell reads -1 here (a finite value whose hundredfold
 *                           leaves the range of int saturates there before it is narrowed).
 *   SLAMHIP_RENDER_PGM      uint8, rows top-down (largest y first), pixels only, no header: what
 *                           GridMapToPgmDumber::dump_map writes behind its header (src/utils/map_dumpers.h:78-87):
 *                           (unsigned char)(255 * (1 - (occ == -1 ? 0.5 : bound_value(0, occ, 1)))); a NaN occupancy
 *                           clamps to 1 as in the reference.
 * value / occ = the cell's GridCell::occupancy().prob_occ: the payload's first double for OCC and GMAPPING cells (a
 * never-observed GMAPPING cell holds -1); for CREDIBILIST o + 0.5 u (TBM_to_O, slams/credibilist/
 * TBM_prob_conversion.h:8-10); for TBM the conversion of the cell CLASS, which the payload does not name -- occ_kind:
 *   SLAMHIP_OCC_TBM_CONSISTENT    TbmOccConsistentCell (tbm_grid_cells.h:89-93): o / (o + e); a cell with the
 *                                 never-updated payload (1, 0, 0) reads 0.5 (the prototype's occupancy).  The
 *                                 reference's cell has that payload too after updates of zero quality only, and reads
 *                                 0 / 0 then: the one case where this value is not the reference's.
 *   SLAMHIP_OCC_TBM_UNKNOWN_EVEN  TbmUnknownEvenOccCell (:104-106): o + 0.5 u
 * occ_kind must be 0 for every other model. */
enum { SLAMHIP_RENDER_OCCGRID = 0, SLAMHIP_RENDER_PGM = 1 };
enum { SLAMHIP_OCC_TBM_CONSISTENT = 0, SLAMHIP_OCC_TBM_UNKNOWN_EVEN = 1 };
/* Window [x0, x0 + w) x [y0, y0 + h) in INTERNAL coordinates of a bound map (like slamhip_map_download_window), out:
 * w * h bytes.  Replaces the cell loops of occupancy_grid_publisher.h:40-46 and map_dumpers.h:78-87 over
 * HipResidentMapView::operator[].  Queued on the context's stream, hence behind every deferred map update; writes
 * nothing to the map.  SLAMHIP_ERR_INVALID (nothing is launched): null out, unknown format, a non-zero occ_kind on a
 * map that is not TBM (or one that is neither kind on a TBM map), a window outside the bound map, an unbound map.
 * While slamhip_profile_enable is on, the kernel's own time is added to slamhip_profile_read's kernel_ms_total. */
int slamhip_map_render(slamhip_ctx *ctx, int map_id, int format, int occ_kind, int x0, int y0, int w, int h,
                       void *out);
/* Host only, no GPU: the same conversion over n cells, payload = n x host stride doubles of cell_model (OCC 1, TBM and
 * CREDIBILIST 4, GMAPPING 3), out = n bytes in cell order.  The kernels and this entry share one definition of the
 * occupancy and of the two byte rules. */
int slamhip_render_cells(int cell_model, int occ_kind, int format, int n, const double *payload, void *out);

/* ---------------------------------------------------------------- scan generation (csrc/scan_generate.hip)
 * LaserScanGenerator::laser_scan_2D (src/utils/data_generation/laser_scan_generator.h:35-80): laser scans ray-cast
 * from a grid map.  For a pose (x, y, theta), a beam angle a, max_dist and occ_threshold:
 *   beam_dir = max_dist * (cos, sin)(a + theta) with the raw provider's libm as the COMPILED reference calls it: the
 *              compiler fuses the cos and the sin of one argument into ONE call of glibc's sincos, whose sine differs
 *              from sin's in the last place now and then (0.855469 <= |x| < 2.426265), and which x86-64 glibc 2.35
 *              does not pick per CPU as it picks sin and cos: restated in csrc/libm_exact.h (sincos_), `variant`
 *              naming the build (0 plain, 1 with FMA contractions) -- slamhip_scan_gen_libm_variant of the host whose
 *              bits are wanted, which need not be its slamhip_libm_variant;
 *   cells    = world_to_cells({robot, robot + beam_dir}), the reference's COMPLETE list (regular_squares_grid.h:56-101):
 *              the 4-connected walk with its tie rule, or Bresenham's list from the start when the walk has not
 *              arrived on the end cell within cells_nm cells -- a hit found early on a walk that later goes astray is
 *              no hit;
 *   in list order, cells with double(map[cell]) < occ_threshold are passed over (cells outside the window are the
 *              prototype cell; a never-observed GMAPPING cell holds -1; the comparison is the reference's, so a NaN
 *              occupancy is NOT below any threshold); the ray is intersected with the bounds of each remaining cell
 *              (Rectangle::find_intersections): 1 intersection = a touch, the list goes on; 2 = the hit, at their
 *              midpoint, range = sqrt(dist_sq(robot, midpoint)).
 * Per beam one status byte and one range (0 unless the status is 1):
 *   0  no hit: the beam adds no point to the scan
 *   1  hit: the scan point (range, a, occupied)
 *   2  the reference would fail an assertion there and stop: another number of intersections
 *      (geometry_primitives.h:392, laser_scan_generator.h:64), or a scan point that world_to_cell(move_origin(...))
 *      does not put back into its cell (:71-74).  No point.
 * The reference's opening assertion (robot on the lower or left boundary of its cell under are_equal, :42-44) is
 * checked on the host for every pose: SLAMHIP_ERR_INVALID for the whole call, nothing is launched.  Also INVALID:
 * poses, angles or max_dist that are not finite, a pose beyond 2^29 cells from the origin, max_dist beyond 2^20 cells,
 * more than 2^26 beams, an occ_kind the map's model does not take (as slamhip_map_render), a variant other than 0 / 1.
 * The host entry and the kernels run ONE per-beam routine (csrc/scan_generate_device.h): equal bits. */
enum { SLAMHIP_SCAN_GEN_SEQUENTIAL = 1 }; /* flags: every beam by the one-thread-per-beam form (the two forms agree
                                           * bit for bit; the default is one wave per beam, 64 walk steps a round) */
/* Which build of glibc's sincos this host's libm runs: 1 FMA, 0 plain, -1 neither (another libm).  Host only. */
int slamhip_scan_gen_libm_variant(int *variant);
/* The generator's angle list (laser_scan_generator.h:47-48): a starts at -half_sector and ACCUMULATES a += angle_inc
 * while a <= half_sector, stopping early when 2 pi <= half_sector + a.  Host only, pose independent.  Writes the first
 * min(*n, cap) angles; *n = the length of the whole list (cap 0, angles NULL: ask for the length). */
int slamhip_scan_gen_angles(double half_sector, double angle_inc, int cap, double *angles, int *n);
/* n_poses x n_angles beams over a bound dense map in one launch; range_out[n_poses][n_angles] doubles, status_out one
 * byte per beam in the same order.  Queued on the context's stream, hence behind every deferred map update; writes
 * nothing to the map; one copy back.  While slamhip_profile_enable is on, the kernel's own time is added to
 * slamhip_profile_read's kernel_ms_total. */
int slamhip_map_generate_scans(slamhip_ctx *ctx, int map_id, int occ_kind, int variant, int flags, int n_poses,
                               const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                               double occ_threshold, double *range_out, unsigned char *status_out);
/* Host only, no GPU: the same beams over a map on the host -- payload[height][width] cells of the model's host stride
 * (OCC 1, TBM and CREDIBILIST 4, GMAPPING 3), unknown_payload = the prototype cell, (origin_x, origin_y) = the internal
 * coordinates of external cell (0, 0). */
int slamhip_scan_generate_host(int cell_model, int occ_kind, int variant, int width, int height, int origin_x, int origin_y,
                               double scale, const double *unknown_payload, const double *payload, int n_poses,
                               const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                               double occ_threshold, double *range_out, unsigned char *status_out);
/* Host only, no GPU: the same beams over ONE tile table in host memory, as slamhip_gmapping_particle_generate_scans
 * (gmapping section) reads a particle's map -- pool[n_tiles][16384][4] GMAPPING cells in 128 x 128-cell tiles (row-major
 * inside a tile, prob_occ first), table[tiles_y * tiles_x] tile ids, (origin_x, origin_y) = the virtual coordinates of
 * external cell (0, 0); a cell outside [0, tiles_x * 128) x [0, tiles_y * 128) reads unknown_occ.  INVALID besides
 * slamhip_scan_generate_host's refusals: a null pool or table, an empty or oversized (> 32768 tiles a side) extent, a
 * table entry outside [0, n_tiles). */
int slamhip_scan_generate_host_tiled(int variant, int tiles_x, int tiles_y, int origin_x, int origin_y, double scale,
                                     double unknown_occ, const double *pool, int n_tiles, const int *table, int n_poses,
                                     const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                                     double occ_threshold, double *range_out, unsigned char *status_out);

/* ---------------------------------------------------------------- map pyramid (csrc/map_pyramid.hip)
 * The two data-parallel parts of the many-to-many multi-resolution matcher (BF_M3RSM, Olson 2015):
 * M3RSMRescalableGridMap (src/core/scan_matchers/m3rsm_engine.h:17-131 over RescalableCachingGridMap,
 * src/core/maps/rescalable_caching_grid_map.h) and Match::prob_upper_bound (m3rsm_engine.h:156-180).  The best-first
 * engine (M3RSMEngine, :238-382) runs on the host over them: slamhip_matcher_create_m3rsm below ("matchers"), which
 * refines a whole layer of matches per launch with slamhip_pyramid_expand_matches (csrc/m3rsm.hip).
 *
 * LEVELS.  Over a bound dense map of model OCC, TBM or CREDIBILIST (the "fine" map, level 0) the pyramid keeps levels
 * 1 .. K, each an ORDINARY bound map with its own map id (first_level_map_id + k - 1), the fine map's cell model and
 * unknown payload, and scale = fine scale doubled k times: slamhip_score_poses, slamhip_map_download_window,
 * slamhip_map_render, ... take a level's id as they take any map's.  Level K is the reference's one cell of infinite
 * scale (rescalable_caching_grid_map.h:35-38): 1 x 1, external cell (0, 0).
 *   The coarse cell at EXTERNAL (X, Y) of level k < K covers the fine external cells (x, y) with floor(x / 2^k) == X and
 *   floor(y / 2^k) == Y (a floor: negative coordinates too); the cell of level K covers every fine cell.  It holds a COPY
 *   of the payload of the known fine cell of largest impact = estimate_obstacle_impact = the per-beam probability of
 *   the scorer for that cell under `oie` (TBM and CREDIBILIST cells: the discrepancy OIE only, as in
 *   slamhip_score_poses); a block without a known fine cell holds the unknown payload.  Equal impacts: the smallest
 *   fine x, then y.  Impacts are compared as numbers, -0 below +0 (NaN impacts, which no valid map holds, by their bits):
 *   a total order, so the result does not depend on how a block is reduced, and two builds give the same bits.
 *   KNOWN means: the payload is not bit-equal to the map's unknown payload.  The resident map has no _is_unknown flag
 *   (grid_cell.h), so a cell that WAS observed and still -- or again -- holds exactly the prototype's payload counts as
 *   unknown here and as known in the reference: the one case where a level cell can differ from the invariant the
 *   reference checks (validate(), m3rsm_engine.h:36-60).
 *   The list of levels is the one ensure_map_cache_is_continuous (rescalable_caching_grid_map.h:171-194) ends with for
 *   a fine map of the same extent whose cells have all been written: levels are added until the last one before the
 *   1 x 1 level is at most 2 x 2 cells, centred on external (0, 0) -- K - 1 = the smallest k >= 0 with
 *   2^k >= max(origin_x, width - origin_x, origin_y, height - origin_y).  A level's window is the tight one around its
 *   blocks (the reference's level windows are centred and grow by Expansion_Rate: supersets, the same cells).
 * Two deliberate differences from the reference:
 *   - the reference never LOWERS a coarse cell (m3rsm_engine.h:96, a TODO): after a fine cell's impact has gone down
 *     its levels keep the old maximum.  The levels here are tight after any history -- a valid and sharper bound;
 *   - the reference skips a propagation when the new impact exceeds the level's by less than ~1e-7 (less_or_equal,
 *     :117-119), so its levels can sit that far below the true maximum.  The levels here hold the exact maximum.
 *
 * create plans and binds the levels (the ids must be free; SLAMHIP_ERR_INVALID for a GMAPPING or unbound fine map, a
 * bad oie, ids out of range) and queues the whole build on the context's stream.  rebuild queues it again -- and plans
 * and binds the levels anew when the fine map has been re-bound (grown) since.  refresh recomputes only the coarse
 * cells whose blocks meet the fine window [x0, x0 + w) x [y0, y0 + h) (INTERNAL coordinates): call it after
 * slamhip_map_append_scan* / slamhip_map_apply_dirty with the window they wrote.  Both are queued on the context's
 * stream, hence behind deferred map updates, and return without waiting.  refresh and the scorer below fail with
 * SLAMHIP_ERR_STATE when the fine map or a level has been re-bound or released behind the pyramid's back.
 * destroy releases the levels and their ids. */
typedef struct slamhip_pyramid slamhip_pyramid;
int slamhip_pyramid_create(slamhip_ctx *ctx, int fine_map_id, int oie, int first_level_map_id, slamhip_pyramid **out);
int slamhip_pyramid_destroy(slamhip_pyramid *pyr);
/* *n_levels = K; entry k - 1 of each array (room for `cap` entries; any pointer may be NULL) = level k */
int slamhip_pyramid_info(slamhip_pyramid *pyr, int *n_levels, int cap, int *map_id, int *width, int *height,
                         int *origin_x, int *origin_y, double *scale);
int slamhip_pyramid_rebuild(slamhip_pyramid *pyr);
int slamhip_pyramid_refresh(slamhip_pyramid *pyr, int x0, int y0, int w, int h);
/* REFRESH OF SEVERAL PYRAMIDS in shared launches (after slamhip_map_append_scan_batch has written K maps).  After the
 * call every level of every pyramid holds, BIT FOR BIT -- payload and winner coordinates -- what slamhip_pyramid_refresh
 * leaves when the same jobs run one after another in job order (tests/test_gpu_pyramid_refresh_batch.py); like the lone
 * call it is queued on the context's stream and does not wait.
 *   A ROUND holds jobs on distinct pyramids (a job naming a pyramid the open round already holds starts the next one).
 *   Per round: one launch per level for the jobs whose window at that level has more than 256 cells (k_pyr_reduce_batch:
 *   a flat grid, the jobs side by side), then ONE launch in which a workgroup per job walks that job's remaining levels up
 *   to the 1 x 1 one (k_pyr_reduce_tail) -- for windows of some hundred cells on 2000 x 2000 maps four or five launches
 *   where K lone calls queue K x 11.  Cell models and OIEs may differ between the jobs.
 *   A pyramid one of whose levels carries a probability plane (a TBM / CREDIBILIST level somebody has scored with the
 *   1-cell OOPE) goes through the lone call at its place in the order (jobs_lone).
 * n_jobs == 0: SLAMHIP_OK, nothing happens.  Refusals, all before anything is queued: SLAMHIP_ERR_INVALID for a null
 * pyramid, one of another context, a window outside its fine map; SLAMHIP_ERR_STATE for a stale pyramid.
 * _stats: the last call that was not refused -- rounds, the jobs that went through the shared launches and through the
 * lone call, and the launches of the rounds (the lone calls' are not counted); any pointer may be NULL. */
typedef struct {
  slamhip_pyramid *pyramid;
  int x0, y0, w, h; /* INTERNAL fine window, as slamhip_pyramid_refresh */
} slamhip_pyramid_refresh_job;
int slamhip_pyramid_refresh_batch(slamhip_ctx *ctx, int n_jobs, const slamhip_pyramid_refresh_job *jobs);
int slamhip_pyramid_refresh_batch_stats(slamhip_ctx *ctx, int *rounds, int *jobs_in_shared_launches, int *jobs_lone,
                                        int *launches);
/* Host only, no GPU: the same levels over a map on the host (payload[height][width] cells of 1 (OCC) or 4 doubles,
 * (origin_x, origin_y) = the internal coordinates of external cell (0, 0)) by the definition the kernels share
 * (csrc/map_pyramid_device.h).  *n_levels = K; the geometry arrays (room for level_cap entries, any may be NULL) as in
 * slamhip_pyramid_info; payload_out (may be NULL: geometry only) receives the levels one after the other, level 1
 * first, each row-major [height_k][width_k][stride]; *payload_need (may be NULL) = the doubles that takes. */
int slamhip_pyramid_build_host(int cell_model, int oie, int width, int height, int origin_x, int origin_y, double scale,
                               const double *unknown_payload, const double *payload, int level_cap, int *n_levels,
                               int *level_width, int *level_height, int *level_origin_x, int *level_origin_y,
                               double *level_scale, size_t payload_cap, double *payload_out, size_t *payload_need);
/* BOUNDS.  Match::prob_upper_bound for n candidates in ONE launch, on the context's current scan.  Candidate i =
 * (rotation[i], rect[i] = bot, top, left, right: its translation rectangle):
 *   level_out[i] = the first k (0 = the fine map) with max(top - bot, right - left) <= scale_k
 *                  (RescalableCachingGridMap::rescale, rescalable_caching_grid_map.h:79-91);
 *   score_out[i] = the scan's probability at pose (x + c.x, y + c.y, rotation[i] + theta), (x, y, theta) = base_pose,
 *                  c = LightWeightRectangle::center() = (left + (right - left) / 2, bot + (top - bot) / 2), on that
 *                  level, with sp_analysis_area = rect[i].
 * cfg->oope must be a window OOPE (max / mean / overlap), cfg->oie the pyramid's; cfg->area is ignored (the rule of
 * cfg->area, at most 10^4 cells per beam, holds by construction: a rectangle is at most one cell of its level wide).
 * Both sum orders; pose_trig DEVICE, HOST or RAW_EXACT.  The value is BIT-EQUAL to slamhip_score_poses on level_out[i]'s
 * map id with cfg.area = rect[i], the same pose_trig and that pose: the same per-beam functions, the same canonical sums.
 *   SLAMHIP_POSE_TRIG_RAW_EXACT is the reference's DEFAULT provider (RawTrigonometryProvider under
 *   LaserScan2D::to_cartesian(rot + pose.theta), m3rsm_engine.h:300-314): a beam's direction is glibc's
 *   cos / sin((rotation[i] + theta) + angle[b]), the sum in the brackets formed first.  It depends on the rotation and the
 *   beam alone, so ONE launch in front of the scoring one tabulates it for the distinct rotations (bit patterns) of the
 *   call and the scoring launch reads its candidate's row; still one scoring launch per call.  Needs the angles of the
 *   current scan's points (slamhip_scan_set_angles / slamhip_scan_filter_upload, or slamhip_scan_select of a slot that
 *   has some): SLAMHIP_ERR_STATE without them, SLAMHIP_ERR_UNSUPPORTED where slamhip_libm_variant is -1 -- both before
 *   anything is launched.
 * SLAMHIP_ERR_INVALID: a rotation, rectangle or base pose that is not finite, bot > top or left > right.
 * _device: rotation, rect, score_out, level_out in HBM, asynchronous on the context's stream, pose_trig DEVICE or
 * RAW_EXACT (a table row per candidate: the host does not see the rotations); a candidate whose rectangle is not finite
 * or is reversed gets NaN and level -1 there. */
int slamhip_pyramid_score_matches(slamhip_ctx *ctx, slamhip_pyramid *pyr, const slamhip_spe_cfg *cfg,
                                  const double base_pose[3], int n, const double *rotation, const double *rect,
                                  double *score_out, int *level_out);
int slamhip_pyramid_score_matches_device(slamhip_ctx *ctx, slamhip_pyramid *pyr, const slamhip_spe_cfg *cfg,
                                         const double base_pose[3], int n, const double *d_rotation, const double *d_rect,
                                         double *d_score_out, int *d_level_out);
/* EXPAND.  The children of n parent matches (rotation[i], rect[i]) made on the device by the reference's refinement rule
 * and bounded as above, in ONE launch (csrc/m3rsm.hip).  The children of a rectangle under `translation_step`
 * (M3RSMEngine::next_best_match / branch, m3rsm_engine.h:318-357, and the matcher's five points,
 * bf_multi_res_scan_matcher.h:55-64), with hb = less(step, right - left), vb = less(step, top - bot),
 * less(a, b) = a < b + DBL_EPSILON (so a side equal to the step still branches) and
 * c = (left + (right - left) / 2, bot + (top - bot) / 2):
 *   hb and vb   4: (bot, c.y, left, c.x), (c.y, top, left, c.x), (bot, c.y, c.x, right), (c.y, top, c.x, right)
 *   hb only     2: (bot, top, left, c.x), (bot, top, c.x, right)          vb only  2: (bot, c.y, ..), (c.y, top, ..)
 *   neither, and not a point (right - left + top - bot > 0)
 *               5: the points (y, y, x, x) at (left, bot), (left, top), (right, bot), (right, top) and c
 *   a point, or a reversed rectangle: none.
 * SLOT LAYOUT.  Every node has 5 child slots, so parent i owns S = 5 (depth 1), 30 (depth 2) or 155 (depth 3) slots,
 * breadth first: slots [0, 5) are its children; slots [5, 30) its grandchildren, slot 5 + 5 a + b being child b of child
 * a; slots [30, 155) the third generation, slot 30 + 25 a + 5 b + c being child c of child b of child a.  Slot s of parent
 * i is entry i * S + s of the outputs: rect_out (4 doubles), score_out, level_out.  A slot without a node (its path
 * meets a node with fewer children) holds a NaN rectangle, a NaN score and level -1.  Every child carries its parent's
 * rotation.  score_out / level_out of a slot with a node are BIT-EQUAL to slamhip_pyramid_score_matches on
 * (rotation[i], rect_out): both kernels run one scoring function.  Both sum orders; pose_trig DEVICE, HOST with one
 * sincos per parent, or RAW_EXACT with one table row per distinct parent rotation (children inherit the rotation; the
 * table, its one launch and its errors as under BOUNDS).  SLAMHIP_ERR_INVALID: depth outside 1..3, a step that is not
 * positive, values that are not finite.
 * _device: everything in HBM, asynchronous on the context's stream, pose_trig DEVICE or RAW_EXACT. */
int slamhip_pyramid_expand_matches(slamhip_ctx *ctx, slamhip_pyramid *pyr, const slamhip_spe_cfg *cfg,
                                   const double base_pose[3], int n, const double *rotation, const double *rect,
                                   double translation_step, int depth, double *rect_out, double *score_out, int *level_out);
int slamhip_pyramid_expand_matches_device(slamhip_ctx *ctx, slamhip_pyramid *pyr, const slamhip_spe_cfg *cfg,
                                          const double base_pose[3], int n, const double *d_rotation, const double *d_rect,
                                          double translation_step, int depth, double *d_rect_out, double *d_score_out,
                                          int *d_level_out);
/* SEVERAL REQUESTS IN ONE LAUNCH.  M3RSMEngine::add_scan_matching_request (m3rsm_engine.h:291-316) may be called any
 * number of times, each call with its own scan, pose and map, and every match of the one queue carries its request's.
 * A request here: a pyramid, a scan kept in HBM by slamhip_scan_store and the pose its drifts are added to.  Candidate
 * (or parent) i of a launch belongs to table[request[i]]; its workgroup takes levels, scan and base pose from that entry
 * (csrc/map_pyramid.hip k_pyr_score_many, csrc/m3rsm.hip k_m3rsm_expand_many) and runs the scoring function of the
 * single-request kernels, so score_out / level_out are BIT-EQUAL to slamhip_pyramid_score_matches /
 * slamhip_pyramid_expand_matches on that request's pyramid, scan (slamhip_scan_select) and pose alone.  Outputs, slot
 * layout, sum orders and pose_trig (HOST: one sincos per candidate / parent, on its own request's heading; RAW_EXACT:
 * one table row per distinct (request, rotation), each over its own request's angles and beam count, filled by one
 * launch in front of the scoring one) as above.  RAW_EXACT needs the angles of every request's slot
 * (slamhip_scan_store_angles): SLAMHIP_ERR_STATE without them, before anything is launched.
 * All pyramids of one call belong to `ctx` and share the cell model and the OIE (= cfg->oie).
 * SLAMHIP_ERR_INVALID: n_requests < 1, a null pyramid or one that is not this context's, mixed cell models or OIEs, a
 * scan slot that holds no scan, a pose that is not finite, a request index outside the table, values that are not
 * finite; SLAMHIP_ERR_STATE: a stale pyramid. */
typedef struct {
  slamhip_pyramid *pyramid;
  int scan_slot;
  double init_pose[3];
} slamhip_m3rsm_request;
int slamhip_pyramid_score_requests(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests,
                                   const slamhip_m3rsm_request *table, int n, const int *request, const double *rotation,
                                   const double *rect, double *score_out, int *level_out);
int slamhip_pyramid_expand_requests(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests,
                                    const slamhip_m3rsm_request *table, int n, const int *request, const double *rotation,
                                    const double *rect, double translation_step, int depth, double *rect_out,
                                    double *score_out, int *level_out);

/* ---------------------------------------------------------------- map update (kernel K6)
 * Replaces GridMapScanAdder::append_scan (src/core/maps/grid_map_scan_adders.h:54-75) with
 * WallDistanceBlurringScanAdder::handle_scan_point (:138-172) and ConstOccupancyEstimator
 * (const_occupancy_estimator.h:6-17) on the HBM mirror: per beam the 4-connected ray walk
 * (regular_squares_grid.h:56-101), per cell the `cell += observation` of the map's cell class, in
 * the reference's update order (records sorted by cell, stable in beam order).
 * rule = which GridCell subclass the OCC/TBM/GMAPPING payload belongs to. */
enum { SLAMHIP_RULE_LAST = 0,     /* GridCell::operator+= (grid_cell.h:27-30): last write wins */
       SLAMHIP_RULE_AFFINE = 1,   /* AffineQualityMergeCell (naive_grid_cells.h:14-20) */
       SLAMHIP_RULE_MEAN = 2,     /* MeanProbabilityCell (naive_grid_cells.h:33-40) */
       SLAMHIP_RULE_TBM = 3,      /* TbmBaseCell (tbm_grid_cells.h:12-19); also CredibilistCell
                                   * (slams/credibilist/grid_cell.h:23-29) on a SLAMHIP_CELL_CREDIBILIST map */
       SLAMHIP_RULE_GMAPPING = 4  /* GmappingBaseCell (gmapping_grid_cell.h:20-33) */ };
typedef struct {
  int rule;
  double scan_quality;                           /* append_scan's scan_quality (x IdleOMQE = 1) */
  double base_occupied_prob, base_occupied_qual; /* slam/occupancy_estimator/base_occupied/{prob,qual} */
  double base_empty_prob, base_empty_qual;       /* .../base_empty/{prob,qual} (init_occupancy_mapping.h:48-51) */
  double blur;                                   /* slam/mapping/blur, metres; < 0 = dynamic */
  double max_range;                              /* slam/mapping/max_range (infinity = unlimited) */
  int occupancy_estimator;  /* slam/occupancy_estimator/type: 0 const (const_occupancy_estimator.h:6-17),
                             * 1 area (AreaOccupancyEstimator, area_occupancy_estimator.h:27-240) */
  double area_shift_amount; /* Q27: the area estimator freezes low_qual * side of the FIRST cell it
                             * ever sees in a function-local static (area_occupancy_estimator.h:68-72);
                             * 0 = 0.01 * scale */
} slamhip_scan_adder_cfg;
/* RAW scan points (range, cos/sin of their angle as for slamhip_scan_upload, is_occupied flag; may
 * be NULL = all occupied).  Every touched cell must lie inside the bound window (grow it with
 * slamhip_map_bind first, or let it grow: slamhip_map_set_auto_grow), otherwise SLAMHIP_ERR_STATE.
 * n_updates = number of cell updates. */
int slamhip_map_append_scan(slamhip_ctx *ctx, int map_id, const slamhip_scan_adder_cfg *cfg,
                            const double pose[3], int n, const double *range, const double *cos_a,
                            const double *sin_a, const int *is_occ, long long *n_updates);
/* The same with a PER-POINT observation quality: the update quality of a cell a beam touches is scan_quality x
 * quality[i] -- GridMapScanAdder::append_scan multiplies by ObservationMappingQualityEstimator::quality(points, pt_i)
 * (grid_map_scan_adders.h:17-43,66-71).  quality = NULL is IdleOMQE (1.0); slamhip_omqe_quality gives the values of
 * the estimators init_omqe builds (init_occupancy_mapping.h:64-80: "idle", "ahr").  The AffineQualityMergeCell,
 * MeanProbabilityCell and TbmBaseCell rules read it; GridCell and GmappingBaseCell ignore an observation's quality. */
int slamhip_map_append_scan_q(slamhip_ctx *ctx, int map_id, const slamhip_scan_adder_cfg *cfg,
                              const double pose[3], int n, const double *range, const double *cos_a,
                              const double *sin_a, const int *is_occ, const double *quality, long long *n_updates);
/* The same from the points' ANGLES, with the reference's DEFAULT trig provider bit for bit: RawTrigonometryProvider
 * evaluates std::cos / std::sin(pose heading + angle) per point (trigonometry_utils.h:17-35; append_scan sets the base
 * angle to the pose's, grid_map_scan_adders.h:61).  The host's libm makes the 2 n values once per scan; the other two
 * entry points take the provider's own table (cos a, sin a) and add the heading by the cached provider's formulas. */
int slamhip_map_append_scan_raw(slamhip_ctx *ctx, int map_id, const slamhip_scan_adder_cfg *cfg, const double pose[3],
                                int n, const double *range, const double *angle, const int *is_occ,
                                const double *quality, long long *n_updates);
/* host helper: ObservationMappingQualityEstimator::quality of every point of a scan (n values): kind 0 IdleOMQE,
 * 1 AngleHistogramResiprocalOMQE = 1 / AngleHistogram::value (grid_map_scan_adders.h:24-43,
 * src/core/features/angle_histogram.h:17-96), over the scan append_scan is given (all its points) */
int slamhip_omqe_quality(int kind, int n, const double *range, const double *angle, double *out);
/* Map updates queued, not awaited (default off).  While on, slamhip_map_append_scan on the zero-copy path returns as
 * soon as the update's kernels are queued on the context's stream -- the scan arrays are consumed before it returns,
 * *n_updates is -1 -- and everything else the context does (matches, scores, downloads, further updates) is ordered
 * behind them: the pose of a scan can be handed on while the GPU still writes that scan into the map
 * (SingleStateHypothesisLaserScanGridWorld::handle_observation, single_state_hypothesis_laser_scan_grid_world.h:52-65,
 * returns only after append_scan).  slamhip_map_drain waits for the queued updates and reports the sum of their cell
 * updates; a failure on the device (a beam outside a window that may not grow) surfaces there as SLAMHIP_ERR_STATE.
 * At most 64 updates stay queued (the 65th drains first); set_deferred(0) drains; a GMapping filter step on the
 * same context drains what is queued into its own count. */
int slamhip_map_set_deferred(slamhip_ctx *ctx, int on);
int slamhip_map_drain(slamhip_ctx *ctx, long long *n_updates);
/* K scans into K resident maps in ONE call: the second half of a K-robot step (the first is
 * slamhip_matcher_process_scan_batch / _raw_scan_batch).  After the call every map holds bit for bit what it would
 * hold after the same jobs went through slamhip_map_append_scan_q (angle == NULL) or slamhip_map_append_scan_raw
 * (angle != NULL) one after another in job order; n_updates[k] is that call's count for job k.
 * The jobs share launches: one k_mu_lines_batch and one k_mu_cells_batch per ROUND (the gather form of the update), a
 * status kernel and one wait.  A round holds jobs on distinct maps; a job naming a map an earlier job of the round
 * names opens the next round, so two robots on one map are applied in job order.  A job the shared launches do not
 * cover -- n > 4096, a key window above 2^22 cells, beam directions that do not ascend within one turn,
 * SLAMHIP_OPT_K6_PATH 1 or 2, a context that is not low-latency, n_jobs == 1 -- runs through the lone call at its
 * place in the order of its map.  Jobs with n <= 0 or every beam range-gated report 0 updates.
 * Maps that may grow (slamhip_map_set_auto_grow) grow by the lone rule, on the host, before their round is launched.
 * cfg->rule must fit the cell model of EVERY job's map; that, null arrays, unknown maps and non-finite end points
 * are found before anything is launched or changed.  A job whose beam leaves a window that may not grow gets
 * status[k] = SLAMHIP_ERR_STATE (its cells inside the window are updated, every other job completes) and the call
 * returns SLAMHIP_ERR_STATE.  The call is awaited, also while slamhip_map_set_deferred is on: it is ordered behind the
 * queued lone updates on the context's stream and leaves them queued (slamhip_map_drain reports them alone). */
typedef struct {
  int map_id;
  double pose[3];
  double scan_quality;          /* replaces cfg->scan_quality for this job (a world sets it per scan) */
  int n;
  const double *range;
  const double *cos_a, *sin_a;  /* as slamhip_map_append_scan_q ... */
  const double *angle;          /* ... or non-NULL: the raw-provider form of slamhip_map_append_scan_raw (cos_a/sin_a ignored) */
  const int *is_occ;            /* may be NULL */
  const double *quality;        /* per point, may be NULL */
  const slamhip_scan_adder_cfg *cfg; /* NULL: the call's cfg.  Else this job's own base probabilities, blur, max_range
                                      * and shift amount (robots whose adders differ still share the launches); its
                                      * rule and occupancy estimator must be the call's, its scan_quality is not read */
} slamhip_map_update_job;
int slamhip_map_append_scan_batch(slamhip_ctx *ctx, const slamhip_scan_adder_cfg *cfg, int n_jobs,
                                  const slamhip_map_update_job *jobs, long long *n_updates /* K */, int *status /* K, may be NULL */);
/* of the last slamhip_map_append_scan_batch: rounds launched, jobs they held, jobs that went through the lone call,
 * kernel launches of the rounds (three per round: lines, cells, status) */
int slamhip_map_update_batch_stats(slamhip_ctx *ctx, int *rounds, int *jobs_in_shared_launches, int *jobs_lone, int *launches);
/* the direction tables the batch keeps per distinct scanner (at most 16, least recently used evicted): how many the
 * context holds, and how many were uploaded since it was created -- a call with known scanners uploads none */
int slamhip_map_update_batch_tables(slamhip_ctx *ctx, int *tables, long long *uploads);
/* update counters of a window (MEAN: n; GMAPPING: hits, tries) -- tests / debugging */
int slamhip_map_download_aux(slamhip_ctx *ctx, int map_id, int x0, int y0, int w, int h, double *out);

/* ---------------------------------------------------------------- scan
 * The FILTERED scan the scorer iterates (LaserScan2D after
 * WeightedMeanPointProbabilitySPE::filter_scan, weighted_mean_point_probability_spe.h:75-95),
 * flattened: per point range, cos/sin of its own angle as the scan's TrigonometryProvider
 * tabulates them, weight (ScanPointWeighting::weight, :21-60) and factor (sensor_data.h:74-75).
 * The arrays are consumed before the call returns; the copy to HBM is queued on the context's stream (no wait for
 * work that is still running there, e.g. a queued map update), ahead of every later score or match. */
int slamhip_scan_upload(slamhip_ctx *ctx, int n, const double *range, const double *cos_a,
                        const double *sin_a, const double *weight, const double *factor);
/* Scans kept RESIDENT in HBM: store copies a filtered scan (arrays as above) into slot `slot` (0..4095) of the
 * context, select makes a stored scan the one the following scores and matches read -- a pointer swap on the
 * host, nothing moves.  For callers that match the same scans repeatedly or several at once
 * (slamhip_matcher_process_scan_batch takes slots as well); a later slamhip_scan_upload replaces the selection,
 * not the stored scans. */
int slamhip_scan_store(slamhip_ctx *ctx, int slot, int n, const double *range, const double *cos_a,
                       const double *sin_a, const double *weight, const double *factor);
int slamhip_scan_select(slamhip_ctx *ctx, int slot);
/* The angles of a STORED scan's points, n = the slot's point count (else SLAMHIP_ERR_INVALID): what
 * SLAMHIP_POSE_TRIG_RAW_EXACT needs of the requests of slamhip_pyramid_score_requests / _expand_requests and of the
 * matches over them.  Kept on the host and in HBM with the slot; a later slamhip_scan_store into the slot drops them;
 * slamhip_scan_select of a slot that has angles makes them the current scan's angles (a slot without angles selects as
 * before: the current scan then has none). */
int slamhip_scan_store_angles(slamhip_ctx *ctx, int slot, int n, const double *angle);
/* The angles of the CURRENT scan's points (ScanPoint2D::angle, sensor_data.h:60-70), n = its point count: what
 * SLAMHIP_POSE_TRIG_RAW_EXACT adds the pose heading to.  Dropped by the next upload / select; slamhip_scan_filter_upload
 * sets them itself. */
int slamhip_scan_set_angles(slamhip_ctx *ctx, int n, const double *angle);
/* Which build of glibc's sin / cos / exp this host's libm runs, found by calling it on arguments where the builds
 * differ: 1 = the FMA build (x86-64 with AVX2 + FMA usable), 0 = the plain build, -1 = neither (another libm): the
 * exact modes (RAW_EXACT, the GMapping OOPE under SLAMHIP_SUM_SEQUENTIAL) then fail with SLAMHIP_ERR_UNSUPPORTED. */
int slamhip_libm_variant(int *variant);
/* the restated functions evaluated ON THE DEVICE (fn 0 sin, 1 cos, 2 exp; variant as above), host arrays in and out:
 * lets a caller (and the tests) confirm device == host libm on its own arguments */
int slamhip_libm_eval(slamhip_ctx *ctx, int variant, int fn, int n, const double *x, double *out);
/* host helpers building cos_a/sin_a: RawTrigonometryProvider (trigonometry_utils.h:17-35) ... */
int slamhip_beam_trig_raw(int n, const double *angle, double *cos_out, double *sin_out);
/* ... and CachedTrigonometryProvider::update + index lookup (trigonometry_utils.h:45-78) */
int slamhip_beam_trig_cached(int n, const double *angle, double a_min, double a_max, double a_inc,
                             double *cos_out, double *sin_out);
/* WeightedMeanPointProbabilitySPE::filter_scan on the host (once per scan, :75-95,136-141).
 * bounded: 1 for PlainGridMap/LazyTiledGridMap (has_cell tests the window), 0 for Unbounded*.
 * cos_a/sin_a as above for the RAW scan; kept_idx receives the raw indices kept. */
int slamhip_filter_scan(int n, const double *range, const double *angle, const int *is_occ,
                        int trig_mode, double a_min, double a_delta, int table_n,
                        const double *tab_sin, const double *tab_cos, const double pose[3],
                        unsigned skip_rate, double max_range, int bounded, int width, int height,
                        int origin_x, int origin_y, double scale, int *kept_idx, int *kept_n);
/* filter_scan + weights + beam trig + slamhip_scan_upload in one call, from the RAW scan (range, angle, is_occ or
 * NULL = all occupied, factor or NULL = all 1.0): what a GridScanMatcher does with a scan before the first candidate
 * is scored (weighted_mean_point_probability_spe.h:75-95; ScanPointWeighting :21-60; trig providers
 * trigonometry_utils.h:17-84).  `bounded`: the map map_id is a PlainGridMap / LazyTiledGridMap whose has_cell()
 * tests the window; 0 for the Unbounded* maps, for which no end point is computed at all (map_id is then not
 * looked at).  Quantities that depend on the beam ANGLES only are kept inside the context until the angle array
 * changes.  weighting: 0 even, 1 viny, 2 ahr; kept_n (may be NULL) = points kept, kept_idx (may be NULL, room for n)
 * their raw indices.  With no point kept nothing is uploaded and scoring fails with SLAMHIP_ERR_STATE (the
 * reference scores such a scan NaN). */
int slamhip_scan_filter_upload(slamhip_ctx *ctx, int map_id, int n, const double *range, const double *angle,
                               const int *is_occ, const double *factor, int trig_mode, double a_min, double a_max,
                               double a_inc, const double pose[3], unsigned skip_rate, double max_range, int bounded,
                               int weighting, int *kept_n, int *kept_idx);
/* How slamhip_scan_filter_upload moves a scan: the per-beam quantities it keeps (cos, sin, the viny weighting's angular
 * factor) are resident in HBM as well, uploaded when the angle array or the trig mode changes; a scan brings its kept
 * ranges, the kept indices where a beam was dropped, and factors / ahr weights where there are any, and a kernel
 * assembles the scan from both.  *uploads = how often the context has uploaded the per-beam tables so far. */
int slamhip_scan_table_uploads(slamhip_ctx *ctx, long long *uploads);
/* The CURRENT scan as the scorers read it, back from HBM (waits for the context's stream): *n = its point count; out5
 * (room for 5 x cap doubles, cap >= *n) receives range, cos, sin, weight, factor as five rows of cap doubles.  With
 * cap 0 only *n is returned. */
int slamhip_scan_download(slamhip_ctx *ctx, int cap, double *out5, int *n);
/* ScanPointWeighting::weight for a filtered scan: kind 0 even, 1 viny, 2 ahr */
int slamhip_scan_weights(int kind, int n, const double *range, const double *angle, double *out);

/* ---------------------------------------------------------------- scoring (kernels K1/K2/K3)
 * Replaces ScanProbabilityEstimator::estimate_scan_probability
 * (src/core/scan_matchers/grid_scan_matcher.h:128-131; WMPP implementation
 * weighted_mean_point_probability_spe.h:97-133) for a BATCH of poses: poses_xyt = n_poses x
 * (x, y, theta) host doubles, scores_out n_poses host doubles (NaN when sum of weights is 0).
 * SLAMHIP_OOPE_GMAPPING scores scans of at most 2048 filtered points (with SLAMHIP_POSE_TRIG_RAW_EXACT: 3840); a longer
 * one is SLAMHIP_ERR_INVALID, "the GMapping kernel holds at most 2048 filtered beams per scan". */
int slamhip_score_poses(slamhip_ctx *ctx, int map_id, const slamhip_spe_cfg *cfg, int n_poses,
                        const double *poses_xyt, double *scores_out);
/* Same with device-resident poses/scores, asynchronous on the context stream (sweep mode) */
int slamhip_score_poses_device(slamhip_ctx *ctx, int map_id, const slamhip_spe_cfg *cfg,
                               int n_poses, const double *d_poses_xyt, double *d_scores_out);
/* The pose sets of K jobs -- K robots, K map hypotheses under one scan, K heat maps -- in ONE call: job k scores its
 * poses over its own map and its own scan, and its n_poses scores land in scores_out behind those of the jobs before it.
 * Job k's scores are BIT-EQUAL to slamhip_scan_select of its slot followed by slamhip_score_poses of its map and
 * poses, in every mode that call has (NaN where the scan's weights add up to 0); they depend neither on the other jobs
 * nor on the route the call takes.  The context's current scan and its angles are what they were before the call.
 *   Shared launches: SLAMHIP_OOPE_OBSTACLE / _MAX / _MEAN / _OVERLAP, both OIEs, OCC / TBM / CREDIBILIST maps (through
 *   the probability plane wherever the lone call goes through it), both sum orders, pose_trig DEVICE and HOST; maps of
 *   any size, scale and origin and scans of any length per job.  One scoring launch per call whatever K; with
 *   SLAMHIP_SUM_SEQUENTIAL a beam-order summing launch behind it.  The jobs' views must share one effective cell model
 *   and OIE (a belief map scored through its plane counts as OCC under the occupancy OIE): else SLAMHIP_ERR_INVALID.
 *   Lone route (select + score, job after job in job order, the current scan put back afterwards):
 *   SLAMHIP_OOPE_GMAPPING (its run cache sees ONE call sequence: the cache ends as the lone calls leave it),
 *   SLAMHIP_POSE_TRIG_RAW_EXACT, a call with a single job that has poses, and a SLAMHIP_SUM_SEQUENTIAL call whose terms
 *   -- the sum of n_poses x scan points over the jobs -- exceed 2^24 doubles (128 MiB of scratch).
 * n_jobs 0 and jobs with n_poses 0 are legal and score nothing (such a job's map and slot are not looked at).  Errors
 * are found before anything is staged or launched and leave scores_out, the stats and the current scan as they were:
 * null arguments, an unknown map, whatever slamhip_score_poses refuses for the configuration, a slot out of range
 * (SLAMHIP_ERR_INVALID); a slot nothing is stored in, scan_slot -1 without a current scan (SLAMHIP_ERR_STATE). */
typedef struct {
  int map_id;
  int scan_slot;           /* 0..4095: a stored scan (slamhip_scan_store); -1: the context's current scan */
  int n_poses;             /* >= 0 */
  const double *poses_xyt; /* n_poses x (x, y, theta), host */
} slamhip_score_job;
int slamhip_score_poses_batch(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_jobs, const slamhip_score_job *jobs,
                              double *scores_out /* sum of n_poses, job after job */);
/* of the last slamhip_score_poses_batch that was not refused: jobs with poses that went through the shared launches,
 * those that went through the lone call, and the kernels the shared route launched to score and sum (1, or 2 with
 * SLAMHIP_SUM_SEQUENTIAL; 0 where every job went lone) */
int slamhip_score_poses_batch_stats(slamhip_ctx *ctx, int *jobs_in_shared_launches, int *jobs_lone, int *launches);
/* GMapping OOPE run-cache state carried between calls (gmapping_occupancy_observation_pe.h:21-24,
 * 36-37,43-44): {cell x, cell y} + cached probability (-1 = empty).  Used by score_poses when
 * cfg->oope == SLAMHIP_OOPE_GMAPPING: poses are scored as ONE call sequence in the given order. */
int slamhip_gm_cache_reset(slamhip_ctx *ctx);
int slamhip_gm_cache_get(slamhip_ctx *ctx, int *cell_xy, double *prob);
int slamhip_gm_cache_set(slamhip_ctx *ctx, const int *cell_xy, double prob);

/* kernel timing of the scoring launches since the last reset (HIP events on the ctx stream) */
int slamhip_profile_enable(slamhip_ctx *ctx, int on);
int slamhip_profile_read(slamhip_ctx *ctx, double *kernel_ms_total, long long *launches,
                         long long *units /* poses x beams launched */, int reset);

/* the same for the map update (K6: count .. apply of one slamhip_map_append_scan or one batched append):
 * recorded HIP events around the pipeline on the context's stream; records = (beam, cell) pairs applied */
int slamhip_profile_read_map_update(slamhip_ctx *ctx, double *ms_total, long long *calls, long long *records,
                                    int reset);

/* ---------------------------------------------------------------- matchers
 * Replace GridScanMatcher::process_scan (src/core/scan_matchers/grid_scan_matcher.h:153-156) of
 *   MonteCarloScanMatcher   (monte_carlo_scan_matcher.h:84-100; enumerator :10-82)
 *   HillClimbingScanMatcher (hill_climbing_scan_matcher.h:128-170; enumerators :10-126)
 *   BruteForceScanMatcher   (brute_force_scan_matcher.h:66-80; enumerator :10-64)
 * through PoseEnumerationScanMatcher::process_scan (pose_enumeration_scan_matcher.h:31-77).
 * The accept/reject chain is evaluated speculatively on the GPU and replayed in the reference's order -- by
 * the next kernel of a device-resident chain (slamhip_matcher_set_device_chain, the default wherever it
 * applies) or, for the configurations the chains do not cover, on the host between batches -- so observers
 * see exactly the reference's event sequence either way. */
typedef struct {
  void *user;
  /* GridScanMatcherObserver (grid_scan_matcher.h:16-32) */
  void (*on_scan_test)(void *user, const double pose[3], double score);
  void (*on_pose_update)(void *user, const double pose[3], double score);
  void (*on_matching_end)(void *user, const double delta[3], double best_score);
} slamhip_observer;

int slamhip_matcher_create_mc(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, unsigned seed,
                              double translation_dispersion, double rotation_dispersion,
                              unsigned failed_attempts_limit, unsigned attempts_limit,
                              slamhip_matcher **out);
int slamhip_matcher_create_hc(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg,
                              unsigned failed_rounds_limit, double translation_delta,
                              double rotation_delta, slamhip_matcher **out);
int slamhip_matcher_create_bf(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const double range9[9],
                              slamhip_matcher **out);
/* BruteForceMultiResolutionScanMatcher (bf_multi_res_scan_matcher.h, BF_M3RSM) over M3RSMEngine (m3rsm_engine.h:252-365):
 * best-first branch and bound over the levels of `pyramid`.  The engine's loop -- std::priority_queue under
 * Match::operator<, add_match's cut, the root layer, next_best_match, the five points of a box that no longer branches,
 * the end at a top that is a point -- runs on the host (csrc/m3rsm_engine.cpp) and takes every score from a memo keyed by
 * (rotation, rectangle).  A child the memo lacks starts a SUPER-STEP: the popped match and the next width - 1 unexpanded
 * entries of the queue are expanded to `depth` generations by one slamhip_pyramid_expand_matches launch.  Scores are
 * pure functions of their node, so the committed calls are the reference's for every width and depth.
 *   cfg: a window OOPE (max / mean / overlap), the pyramid's OIE, pose_trig DEVICE, HOST or RAW_EXACT.  With
 *   SLAMHIP_SUM_SEQUENTIAL the match is the compiled reference's bit for bit -- delta, probability and every call --
 *   under HOST trig for scans under the cached trig provider, and under RAW_EXACT for scans under the reference's
 *   default provider (RawTrigonometryProvider, use_trig_cache = false; the scan's cos_a / sin_a are then not read, its
 *   angles are: slamhip_scan_set_angles, slamhip_scan_filter_upload or a raw scan).  The default mode's scores differ by
 *   the sum order (~1e-13).  RAW_EXACT adds one small tabulation launch in front of every root and expand launch (the
 *   exact directions of the launch's distinct rotations) and nothing else; the many-to-many and each forms below take
 *   it too, given slamhip_scan_store_angles for every request's slot.
 *   process_scan / process_raw_scan: map_id must be the pyramid's fine map; delta = (centre x, centre y, rotation) of
 *   the winning point, prob = its bound; on_matching_end is the only observer event (the reference's matcher emits no
 *   on_scan_test).  slamhip_matcher_stats: scorer_calls = the calls the reference would have made, poses_evaluated =
 *   candidates scored on the GPU, launches = super-steps + the root launch.
 * SLAMHIP_ERR_INVALID: a 1-cell or GMapping OOPE, an OIE that is not the pyramid's, a pyramid of another context, steps
 * that are not positive; SLAMHIP_ERR_STATE from a match: the pyramid is stale (slamhip_pyramid_rebuild), or RAW_EXACT
 * without the scan's angles (nothing is launched, the stats of the match before stay);
 * SLAMHIP_ERR_UNSUPPORTED from a match: the bound on super-steps (2^20) was reached.  The pyramid must outlive the matcher. */
int slamhip_matcher_create_m3rsm(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, slamhip_pyramid *pyramid,
                                 double max_x_error, double max_y_error, double max_th_error, double angle_step,
                                 double translation_step, slamhip_matcher **out);
/* parents per expand launch (>= 1) and generations per parent (1..3); default 32, 3 -- the
 * fastest point of the grid tools/m3rsm_ms.py measures.  (0, 0): no expand launches at
 * all -- every popped match's children are split on the host and bounded by one slamhip_pyramid_score_matches launch, a
 * round trip per pop: the route the speculation is measured against (tools/m3rsm_ms.py).  Same trace either way. */
int slamhip_matcher_set_m3rsm_speculation(slamhip_matcher *m, int width, int depth);
/* The committed scorer calls of the last match in the reference's order: row k of rows (room for cap rows of 7
 * doubles) = rotation, bot, top, left, right, score, level; *n = how many there were (may exceed cap). */
int slamhip_matcher_m3rsm_trace(slamhip_matcher *m, int cap, double *rows, int *n);
/* MANY-TO-MANY: several requests in ONE search, as the reference's engine takes them (add_scan_matching_request once per
 * request, m3rsm_engine.h:291-316; then BruteForceMultiResolutionScanMatcher::process_scan's loop,
 * bf_multi_res_scan_matcher.h:44-65).  The root layers are committed request by request in the order given -- all of
 * them bounded in one slamhip_pyramid_score_requests launch --; there is one queue and one best finest probability, so
 * a good point of one request prunes the others; a super-step's parents come from the shared queue whatever request
 * they belong to (slamhip_pyramid_expand_requests).  The first popped match that is a point wins:
 * *out_request = its request, out_delta = (centre x, centre y, rotation), *out_prob = its bound -- the request whose
 * lone match has the largest probability, in fewer calls than the lone matches together.  The matcher's limits, steps,
 * cfg and speculation apply to every request; the matcher's own pyramid takes no part.  Stats and observer
 * (on_matching_end once) as for a lone match.  If every bound is NaN: *out_request = -1, delta 0, prob NaN.
 * SLAMHIP_ERR_INVALID / _STATE as for slamhip_pyramid_score_requests. */
int slamhip_matcher_m3rsm_match_many(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req,
                                     int *out_request, double out_delta[3], double *out_prob);
/* The committed calls of the last slamhip_matcher_m3rsm_match_many: rows of 8 doubles = request, rotation, bot, top,
 * left, right, score, level; cap and *n as for slamhip_matcher_m3rsm_trace. */
int slamhip_matcher_m3rsm_trace_many(slamhip_matcher *m, int cap, double *rows, int *n);
/* K INDEPENDENT matches in one call -- K robots or replicas --: request k = (pyramid, stored scan slot, pose), K answers.
 * Every request has its own search (queue, best finest probability, memo); the searches advance in LOCK-STEP and share
 * nothing but the launches: all root layers in one slamhip_pyramid_score_requests launch, then rounds -- every search
 * that needs children the memo lacks hands over its popped match and its own width - 1 ride-alongs, the parents of all
 * of them go, in request order, into ONE slamhip_pyramid_expand_requests launch, every search takes its slice and runs
 * on; a search that has ended takes no further part.  1 + (the longest search's super-steps) launches instead of the sum
 * over requests; between two launches the searches run on worker threads (slamhip_matcher_set_m3rsm_threads).
 *   out_deltas[3 k ..], out_probs[k]: what a lone slamhip_matcher_process_scan gives -- a matcher with this cfg, these
 *   limits, steps and speculation over req[k].pyramid, slot req[k].scan_slot selected, at req[k].init_pose --, bit for
 *   bit in both sum orders: delta, probability, committed calls and counters.  A request whose search finds nothing gets
 *   what the lone call makes of that (delta 0, prob NaN, no observer call); the other requests are not affected.
 *   The matcher's limits, steps, cfg and speculation apply to every request; its own pyramid takes no part.  The same
 *   slot or pyramid may appear in several requests.  Observer: on_matching_end once per request that has a match, in
 *   request order, after the searches.  slamhip_matcher_stats: scorer_calls and poses_evaluated summed over the requests,
 *   launches = the launches made.  With SLAMHIP_SUM_SEQUENTIAL a launch stages slots x beams doubles of terms per
 *   candidate; a round whose terms would exceed 256 MiB goes as consecutive launches in request order (same results).
 *   slamhip_matcher_m3rsm_trace / _trace_many are NOT defined after this call: use slamhip_matcher_m3rsm_trace_each.
 * SLAMHIP_ERR_INVALID / _STATE as for slamhip_matcher_m3rsm_match_many, found before anything is launched; also
 * SLAMHIP_ERR_INVALID: not a BF_M3RSM matcher; speculation (0, 0) (the per-pop measuring route has no batched form).
 * SLAMHIP_ERR_UNSUPPORTED: a request reached the bound on super-steps (no outputs then).
 * slamhip_matcher_process_scan_batch / _process_raw_scan_batch keep refusing a BF_M3RSM matcher. */
int slamhip_matcher_m3rsm_match_each(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req,
                                     double *out_deltas /* 3 per request */, double *out_probs);
/* Request `request` of the last slamhip_matcher_m3rsm_match_each: its committed calls (rows as for
 * slamhip_matcher_m3rsm_trace) and its counters -- scorer_calls, poses_evaluated as slamhip_matcher_stats reports them
 * after the lone match, the super-steps it took part in and its branching pops.  Null outputs are skipped. */
int slamhip_matcher_m3rsm_trace_each(slamhip_matcher *m, int request, int cap, double *rows /* 7 per row */, int *n);
int slamhip_matcher_m3rsm_each_stats(slamhip_matcher *m, int request, long long *scorer_calls,
                                     long long *poses_evaluated, long long *super_steps, long long *branching_pops);
/* worker threads of slamhip_matcher_m3rsm_match_each's host half: 1 .. 16 (1: the calling thread alone), 0 = the default,
 * min(requests, 8).  Results do not depend on it. */
int slamhip_matcher_set_m3rsm_threads(slamhip_matcher *m, int threads);
/* Scan point weights that turn with the candidate's ROTATION.  The reference's matcher hands its estimator PREROTATED scans
 * (prerotate_scan = true, bf_multi_res_scan_matcher.h:42-43): Cartesian points in the world's orientation, and a weighting
 * that reads a point's angle() -- VinySlamSPW, weighted_mean_point_probability_spe.h:47-60 -- weighs it by beam angle +
 * rotation + heading.  `even` weights do not depend on the point and need none of this.
 *   slamhip_matcher_m3rsm_rotations: the distinct rotations of the root layer in its order (0, -s, +s, -2 s, ...;
 *   *n = how many, may exceed cap).
 *   slamhip_matcher_set_m3rsm_rotation_slots(m, 1): from now on a request's scan_slot is the FIRST of *n consecutive slots,
 *   slot scan_slot + j holding the scan -- the same points -- with the weights under rotation j of that list (and its angles,
 *   for RAW_EXACT); a candidate reads the slot of its rotation.  The search, its calls and its counters are otherwise those
 *   of slamhip_matcher_m3rsm_match_many / _match_each; a missing slot is SLAMHIP_ERR_INVALID before anything is launched.
 *   While on, slamhip_matcher_process_scan / _process_raw_scan are refused (SLAMHIP_ERR_INVALID): the current scan has one
 *   set of weights.  A lone match is match_many over one request. */
int slamhip_matcher_m3rsm_rotations(slamhip_matcher *m, int cap, double *rotation, int *n);
int slamhip_matcher_set_m3rsm_rotation_slots(slamhip_matcher *m, int on);
/* Bytes the launches of the last BF_M3RSM match -- lone, many-to-many or each -- wrote back to the host: 12 per root
 * candidate (score, level), 44 per slot of every parent (rectangle, score, level), slots without a node included. */
int slamhip_matcher_m3rsm_copied_back(slamhip_matcher *m, long long *bytes);
int slamhip_matcher_destroy(slamhip_matcher *m);
/* GridScanMatcher::reset_state (grid_scan_matcher.h:158) */
int slamhip_matcher_reset_state(slamhip_matcher *m);
int slamhip_matcher_set_observer(slamhip_matcher *m, const slamhip_observer *obs);
/* max speculative poses per launch (0 = default) */
int slamhip_matcher_set_batch(slamhip_matcher *m, int max_batch);
/* Hill climbing (1-cell or GMapping OOPE) and Monte Carlo (1-cell OOPE) with device pose trigonometry run their
 * whole accept chain on the device: one process_scan = a chain of kernels with no host in between, each replaying
 * the previous one's speculative candidates in the reference's order (csrc/hc_chain.h, csrc/mc_chain.h;
 * pose_enumeration_scan_matcher.h:31-77, hill_climbing_scan_matcher.h:10-170, monte_carlo_scan_matcher.h:10-100).
 * mode: 0 = the host-driven speculative batches every other configuration uses; 1 = a chain of kernels, one per
 * super-step; 2 (default) = the match as ONE launch whose workgroups stay on the chip and exchange their scores
 * inside it -- hill climbing over the 1-cell and window OOPEs (csrc/hc_resident.hip), Monte Carlo
 * (csrc/mc_resident.hip), and, when asked for explicitly, hill climbing over the GMapping OOPE
 * (csrc/hc_resident_gm.hip; by default a lone GMapping chain stays on mode 1, which is as fast).  Every wait in
 * that launch is bounded, and a match whose workgroups were not all resident (the device was shared) is redone by
 * mode 1, as is everything mode 2 does not cover; threads: workgroup size 256 / 512 / 1024, 0 = default (1024 for
 * hill climbing, 512 for Monte Carlo).  Scores, decisions, observer events and the Monte-Carlo engine's stream are
 * the same bit for bit in every mode. */
int slamhip_matcher_set_device_chain(slamhip_matcher *m, int mode, int threads);
/* mode 2's bookkeeping: matches launched in the co-resident form, and how many of them gave up (bounded wait ran
 * out) and were redone by the chain of kernels */
int slamhip_matcher_resident_stats(slamhip_matcher *m, long long *matches, long long *gave_up);
/* The default mode (SLAMHIP_SUM_TREE256) over the 1-cell AND the window OOPEs (max / mean / overlap: r05) is CHECKED
 * (on = 1, the default) in every form -- co-resident launch, chain of kernels, host-driven batches, brute-force
 * sweep: a `best < candidate` (pose_enumeration_scan_matcher.h:58) between canonical tree sums that lie within 2^-40
 * of each other -- more than the two orders of summation can differ by -- and whose beam terms are not identical
 * (compared through a fingerprint of the term vector) is not decided from the tree sums: the poses in question are
 * summed once more in the reference's beam order (weighted_mean_point_probability_spe.h:108-124) and those sums
 * decide.  The accept chain is then the one SLAMHIP_SUM_SEQUENTIAL gives, at the default mode's speed; reported
 * scores stay the canonical sums.  on = 0: decisions from the tree sums as they are (ties between mathematically
 * equal candidates can then fall the other way: 4 of 200 fuzzed matches over the 1-cell OOPE, 2 of 200 over `max`,
 * tests/test_gpu_hc_chain.py).
 * The GMapping OOPE (r06): a lone matcher's default mode is checked too, by another mechanism -- its per-beam value is
 * exp() of a distance and the fast paths use the device's exp, so there are no beam-order sums of the SAME terms to
 * re-decide from.  A comparison on the walked path whose two scores lie within 2^-40 of each other (two zero scores
 * excepted) is reported before anything has been shown to an observer (device chains: error 7; host-driven batches:
 * MatchJob::gm_unsettled), and the whole match is redone in the EXACT mode: call order, beam-order sums, glibc's exp
 * restated (csrc/libm_exact.h, exact_kernels.hip), with the reference's default RawTrigonometryProvider where the
 * context knows the scan's angles (slamhip_scan_set_angles / slamhip_scan_filter_upload), else the cached provider's
 * angle addition.  Redone matches are counted in slamhip_matcher_chain_stats' steps_rescored.  At the limits GMapping
 * uses (6 failed rounds, init_gmapping.h:58-60) no comparison comes that close and nothing is redone; at limit 27 --
 * steps of 7e-10 m around an optimum -- nearly every match is, and takes the reference's accept path
 * (tests/test_gpu_hc_chain.py).  The filter's per-particle chains (slamhip_gmapping_*) are not checked: they run
 * GMapping's hard-wired limit, and their exact form is SLAMHIP_POSE_TRIG_RAW_EXACT. */
int slamhip_matcher_set_tie_check(slamhip_matcher *m, int on);
/* process_scan on the currently uploaded (filtered) scan; out_delta = best - init */
int slamhip_matcher_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3],
                                 double out_delta[3], double *out_prob);
/* GridScanMatcher::process_scan as the reference declares it (grid_scan_matcher.h:153-156,
 * pose_enumeration_scan_matcher.h:31-77): the RAW scan in -- filter_scan against init_pose (:38), the scan-point weights
 * and the beam trigonometry, the copy to HBM (everything slamhip_scan_filter_upload does, same arguments, gathered in
 * slamhip_raw_scan) -- and the match, in one call.  *kept_n (may be NULL) = points filter_scan kept.  With no point
 * kept the reference's scorer returns 0 / 0 for every candidate and nothing is ever accepted: *out_prob = NaN,
 * out_delta = 0, no launch (observers are not called for such a scan). */
typedef struct slamhip_raw_scan {
  int n;
  const double *range, *angle;
  const int *is_occ;     /* NULL: every point occupied */
  const double *factor;  /* NULL: all 1.0 */
  int trig_mode;         /* SLAMHIP_TRIG_RAW / _CACHED (+ a_min, a_max, a_inc of the cached provider) */
  double a_min, a_max, a_inc;
  unsigned skip_rate;
  double max_range;
  int bounded;           /* see slamhip_scan_filter_upload */
  int weighting;         /* 0 even, 1 viny, 2 ahr */
} slamhip_raw_scan;
int slamhip_matcher_process_raw_scan(slamhip_matcher *m, int map_id, const slamhip_raw_scan *scan,
                                     const double init_pose[3], double out_delta[3], double *out_prob, int *kept_n);
/* K independent matches in shared launches -- PoseEnumerationScanMatcher::process_scan
 * (pose_enumeration_scan_matcher.h:31-77) once per robot / replica (the single-hypothesis matchers do not
 * shard, they replicate): match k = (filtered scan k, initial pose k, map k).  Every match gets the result, the
 * accept trace and the counters of a lone slamhip_matcher_process_scan on the same inputs, bit for bit; what changes
 * is how the GPU is used: a lone hill-climbing match is a chain of ~16 dependent kernels of 253 one-pose workgroups
 * (latency-bound, a quarter of the chip), K of them advance together, one super-step per kernel (grid.y = match,
 * map and scan from a job table in HBM), with trees sized so that all matches' candidates fill the CUs.  Covers
 * what the device chain covers (hill climbing, 1-cell OOPE, default mode, OCC or TBM maps of one cell model);
 * anything else -- and a batch of one -- runs the matches one after another through slamhip_scan_upload +
 * slamhip_matcher_process_scan (the context's uploaded scan is unspecified after the call).  The matcher's
 * observer, if set, sees the matches' event sequences one after another, job 0 first, each closed by
 * on_matching_end.  out_deltas: 3 doubles per job; out_probs: one. */
typedef struct {
  int map_id;
  int scan_slot;                            /* >= 0: the scan stored in that slot (slamhip_scan_store), resident in
                                             * HBM -- n and the arrays below are ignored; -1: the arrays below */
  int n;                                    /* beams of the filtered scan, arrays as for slamhip_scan_upload */
  const double *range, *cos_a, *sin_a, *weight;
  const double *factor;                     /* may be NULL = all 1.0 */
  double init_pose[3];
} slamhip_match_job;
int slamhip_matcher_process_scan_batch(slamhip_matcher *m, int n_jobs, const slamhip_match_job *jobs,
                                       double *out_deltas, double *out_probs);
/* counters of job `job` of the last batch (slamhip_matcher_stats gives the sums; its `launches` the longest
 * chain's super-steps); on_device_chain: 1 when the match ran in the shared launches */
int slamhip_matcher_batch_stats(slamhip_matcher *m, int job, long long *scorer_calls, long long *poses_evaluated,
                                long long *super_steps, int *on_device_chain);
/* K RAW scans in, K matches in the shared launches: slamhip_matcher_process_raw_scan for K robots / replicas.  Per job
 * the host runs the lone call's filter against the job's map window and initial pose and makes the ahr weights; what
 * is new with each scan (kept ranges, kept indices where a beam was dropped, factors where given, ahr weights) goes
 * into ONE pinned arena, one kernel launch assembles all the scan blocks in HBM from it and from per-beam tables kept
 * resident per distinct scanner (n, angles, trig_mode, a_min / a_max / a_inc: jobs with equal scanners share a table, a
 * later call with the same scanners uploads none -- slamhip_scan_table_uploads counts these uploads too), and the
 * chains of slamhip_matcher_process_scan_batch run behind it.
 *  - Per-job results: job k gets the delta, probability, kept count (kept_n[k]; kept_n may be NULL), observer event
 *    sequence and slamhip_matcher_batch_stats counters of a lone slamhip_matcher_process_raw_scan on the same inputs,
 *    bit for bit.  Observer sequences run job 0 first, each closed by on_matching_end.
 *  - A job whose filter keeps no point is what the lone call makes of it: probability NaN, delta 0, no observer call.
 *    It takes no part in the launches; the other jobs are unaffected.
 *  - Jobs the chains do not cover run one after another through the lone raw call, in job order (a Monte-Carlo
 *    matcher's engine stream is that of the sequence of lone calls, unless it has engine streams of its own:
 *    slamhip_matcher_set_mc_streams below): a matcher that is neither hill climbing nor Monte Carlo with streams, a window or
 *    GMapping OOPE, the beam-order sum, a job with more than 4096 kept points, n_jobs == 1 (or one non-empty job).
 *  - Errors are those of slamhip_matcher_process_scan_batch and of the lone raw call -- unknown map, maps of different
 *    cell models (or GMAPPING cells) in the shared launches, a trig_mode that is neither provider, an angle outside
 *    the cached provider's table, n <= 0, null arrays, an unknown weighting --, found before anything is launched; the
 *    matcher's last-batch state (slamhip_matcher_batch_stats) stays that of the batch before.
 *  - Stored scan slots are never touched.  The context's selected or uploaded scan is not touched by the shared
 *    launches; where a job went through the lone call, a selected slot is selected again afterwards and an uploaded
 *    scan is invalidated (its buffer has been overwritten), as slamhip_matcher_process_scan_batch leaves them.
 *  - A BF_M3RSM matcher is refused (SLAMHIP_ERR_INVALID), as by slamhip_matcher_process_scan_batch. */
typedef struct {
  int map_id;
  slamhip_raw_scan scan;   /* as for slamhip_matcher_process_raw_scan */
  double init_pose[3];
} slamhip_raw_match_job;
int slamhip_matcher_process_raw_scan_batch(slamhip_matcher *m, int n_jobs, const slamhip_raw_match_job *jobs,
                                           double *out_deltas, double *out_probs, int *kept_n);
/* job's scan block of the last raw batch, as slamhip_scan_download gives the current scan: *n = its kept count, out5
 * five rows of cap doubles (cap 0: only *n).  A job that went through the lone call has no block in the batch's arena:
 * *n is set, asking for the rows is an error. */
int slamhip_matcher_batch_scan_download(slamhip_matcher *m, int job, int cap, double *out5, int *n);
/* K RAW scans in, K MULTI-RESOLUTION matches: the raw-scan form of slamhip_matcher_m3rsm_match_each (a BF_M3RSM matcher
 * only; the two batch calls above keep refusing one).  Per request the host runs the lone call's filter against the
 * window of the request's pyramid's FINE map and the initial pose; what is new with each scan goes into ONE pinned arena
 * of the matcher's own, ONE launch (k_scan_assemble_table) assembles every live request's block in HBM -- the five rows
 * and, as a sixth, the kept points' angles (SLAMHIP_POSE_TRIG_RAW_EXACT reads them) -- from per-scanner tables kept
 * resident between calls (slamhip_scan_table_uploads counts their uploads: a second call with the same scanners sends
 * none), and the lock-step searches of slamhip_matcher_m3rsm_match_each run over those blocks.
 *  - Request k gets what a lone slamhip_matcher_process_raw_scan gives it on a matcher with this cfg, these limits, these
 *    steps and this speculation over req[k].pyramid, with map_id = that pyramid's fine map, the same slamhip_raw_scan and
 *    the same pose: delta, probability, kept count (kept_n[k]; kept_n may be NULL), committed calls
 *    (slamhip_matcher_m3rsm_trace_each) and counters (slamhip_matcher_m3rsm_each_stats), BIT FOR BIT, in both sum
 *    orders, under pose_trig DEVICE, HOST and RAW_EXACT, for every weighting, both scan trig providers and every thread
 *    count (tests/test_gpu_m3rsm_each_raw.py).
 *  - A request whose filter keeps nothing: probability NaN, delta 0, kept 0, no observer call, zero counters, an empty
 *    trace; it takes no part in the launches.  If every request is empty nothing is launched.  The observer gets
 *    on_matching_end once per request that has a match, in request order.
 *  - slamhip_matcher_stats: launches = slamhip_matcher_m3rsm_match_each's count + 1 (the assembly launch); 0 when
 *    nothing was launched.
 *  - Stored scan slots, the selected slot and an uploaded scan are not touched.  n_requests == 1 takes the same path.
 *  - Refusals, all before anything is launched or the last call's state is replaced: SLAMHIP_ERR_INVALID for a matcher
 *    that is not BF_M3RSM, speculation (0, 0), rotation slots on (rotation-slot scans are not made on the device: their
 *    viny / ahr weights turn with the candidate), a null or foreign pyramid, pyramids of different cell models or OIEs,
 *    and whatever the lone raw call and slamhip_matcher_process_raw_scan_batch refuse of a scan; SLAMHIP_ERR_STATE for
 *    a stale pyramid; RAW_EXACT on a host whose libm is neither restated build: the code the stored form gives. */
typedef struct {
  slamhip_pyramid *pyramid; /* the scan is filtered against the fine map this pyramid stands over */
  slamhip_raw_scan scan;    /* as for slamhip_matcher_process_raw_scan */
  double init_pose[3];
} slamhip_m3rsm_raw_request;
int slamhip_matcher_m3rsm_match_each_raw(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_raw_request *req,
                                         double *out_deltas /* 3 per request */, double *out_probs, int *kept_n);
/* request's scan block of the last such call, as slamhip_matcher_batch_scan_download gives a job's; angle_out (may be
 * NULL) the kept points' angles */
int slamhip_matcher_m3rsm_each_scan_download(slamhip_matcher *m, int request, int cap, double *out5, double *angle_out, int *n);
/* K robots' engines on ONE Monte-Carlo matcher.  In the reference every robot owns its matcher and with it an engine of
 * its own seed (init_scan_matching.h:118-135); a matcher has one std::mt19937, never reseeded, so the batch calls above
 * run a Monte-Carlo matcher's jobs one after another on that one engine.  With streams set, the two batch calls run job
 * j on ITS stream -- in shared launches (grid.y = job, one kernel = one super-step of every chain still alive), at most
 * S = min(511, failed limit, attempts limit, 2048 / K - 1) candidates per job and super-step (a speed knob: results do
 * not depend on it) -- and job j gets the result, the observer sequence and the counters of a lone matcher created with
 * seeds[stream] and fed that stream's jobs in order, bit for bit.
 *  - Stream k is what slamhip_matcher_create_mc(..., seeds[k], ...) with this matcher's dispersions and limits would
 *    own: GaussianPoseEnumerator{mt19937(seed)} (monte_carlo_scan_matcher.h:14-37).  It is never reseeded and carries on
 *    from batch call to batch call.  n_streams = 0 removes the streams; setting them anew restarts all of them and drops
 *    the job mapping.  A matcher that is not Monte Carlo: SLAMHIP_ERR_INVALID.
 *  - slamhip_matcher_reset_state resets every stream's enumerator as it resets the matcher's own; the engines stay
 *    where they are.
 *  - A matcher without streams behaves in every entry point as it did before these calls existed; a matcher with
 *    streams changes only the two batch calls: lone slamhip_matcher_process_scan / _process_raw_scan keep using the
 *    matcher's own engine.
 *  - The shared launches cover what the lone Monte-Carlo chain covers (1-cell OOPE, device pose trigonometry, maps of one
 *    cell model) in the default sum order.  Jobs they do not cover run the lone path ON THEIR OWN STREAM, in job order:
 *    the beam-order sum, more than 4096 kept points, an observer trace that outgrows its buffer, n_jobs == 1 (or one
 *    non-empty job).  A job's result never depends on the route; slamhip_matcher_batch_stats says which it took.
 *  - A raw job whose filter keeps nothing does not advance its stream (NaN, zero delta, no observer call).
 *  - Errors found before anything is launched -- unknown map, maps of different cell models, a bad stream mapping, null
 *    arrays -- leave every stream and the last-batch state untouched.  After a HIP failure in flight the streams'
 *    positions are unspecified. */
int slamhip_matcher_set_mc_streams(slamhip_matcher *m, int n_streams, const unsigned *seeds);
/* which stream job j of the NEXT batch calls uses.  NULL or n = 0: identity (job j on stream j).  Two jobs on one stream,
 * a stream out of range, more jobs than streams: SLAMHIP_ERR_INVALID, here (the mapping stays what it was) and again in a
 * batch call with more jobs than the mapping names -- before anything is staged or launched, no stream touched. */
int slamhip_matcher_set_mc_job_streams(slamhip_matcher *m, int n, const int *stream_of_job);
/* a stream's engine and enumerator: absolute position on its pair tape (Marsaglia pairs drawn since the seed), matches
 * run on it, and state5 = (failed, poses, translation dispersion, rotation dispersion, has_saved) -- may be NULL.
 * stream = -1: the matcher's own enumerator, the one the lone calls use. */
int slamhip_matcher_mc_stream_info(slamhip_matcher *m, int stream, unsigned long long *pairs_consumed,
                                   long long *matches, double *state5);
/* K robots' enumerators on ONE brute-force matcher.  In the reference every robot owns its matcher, and a
 * BruteForcePoseEnumerator latches the pose it is given at the FIRST next() of its life as its base and never clears it
 * (brute_force_scan_matcher.h:27-40).  With one matcher every job of a batch therefore enumerates around the first job's
 * first initial pose: right for a sequence of lone calls on one matcher, not what K robots with K matchers compute.
 * With streams set, the two batch calls run job j on ITS stream, all jobs in three shared launches for any K (score,
 * scan, decide, grid.y = job; the raw form's assembly launch in front makes four), and job j gets the delta, the
 * probability, the observer sequence, the counters (scorer calls = 1 + nx ny nt) and, for raw jobs, the kept count of a
 * lone brute-force matcher with the same configuration and range9, fed that stream's jobs in order, bit for bit.
 *  - Stream k is what slamhip_matcher_create_bf with this matcher's range9 would own: the same offsets and an UNLATCHED
 *    base.  n_streams = 0 removes the streams; setting them anew forgets every base and drops the job mapping.  A matcher
 *    that is not brute force: SLAMHIP_ERR_INVALID.
 *  - slamhip_matcher_reset_state rewinds every stream as it rewinds the matcher's own enumerator; latched bases stay, as
 *    the reference's reset() leaves them.
 *  - A matcher without streams behaves in every entry point as it did before these calls existed (its batch jobs run
 *    job after job through the lone call, slamhip_matcher_batch_stats reports on_device_chain = 0); a matcher with
 *    streams changes only the two batch calls: lone slamhip_matcher_process_scan / _process_raw_scan keep using the
 *    matcher's own enumerator.
 *  - The shared launches cover what the lone sweep covers over the 1-cell OOPE: the default sum order, device pose
 *    trigonometry, a low-latency context, the device chain not switched off, maps of one cell model (TBM and
 *    CREDIBILIST maps through their probability plane wherever the lone call goes through it).  What they do not cover
 *    runs the lone call ON THE JOB'S OWN STREAM, in job order: window OOPEs, the GMapping OOPE, the beam-order sum, host
 *    pose trigonometry, n_jobs == 1 (or one non-empty raw job), a job above 4096 beams (that job alone in the array
 *    form; every job of a raw batch), and a call whose K x (1 + nx ny nt) poses exceed the scratch budget of 2^24 poses
 *    (the launches keep a score, a fingerprint and a prefix index, 24 bytes, per pose: 384 MiB at the budget; a sweep
 *    itself holds at most 2^26 poses).  A job whose walk meets a comparison the tree sums cannot settle (the checked
 *    default mode) is redone alone by the host-driven route on its stream; the other jobs keep their results.  A job's
 *    result never depends on the route; slamhip_matcher_batch_stats says which it took.
 *  - A raw job whose filter keeps nothing is NaN, zero delta, no observer call, and does NOT latch its stream's base.
 *  - Errors found before anything is launched -- unknown map, maps of different cell models, GMAPPING cells, a bad
 *    stream mapping, null arrays -- leave every stream's base and the last-batch state untouched. */
int slamhip_matcher_set_bf_streams(slamhip_matcher *m, int n_streams);
/* which stream job j of the NEXT batch calls uses.  NULL or n = 0: identity (job j on stream j).  Two jobs on one stream,
 * a stream out of range, more jobs than streams: SLAMHIP_ERR_INVALID, here (the mapping stays what it was) and again in a
 * batch call -- before anything is staged, launched or latched. */
int slamhip_matcher_set_bf_job_streams(slamhip_matcher *m, int n, const int *stream_of_job);
/* a stream's enumerator: whether its base is latched, the base (zeros while it is not), the matches run on it.  Outputs
 * may be NULL.  stream = -1: the matcher's own enumerator, the one the lone calls use. */
int slamhip_matcher_bf_stream_info(slamhip_matcher *m, int stream, int *base_set, double base[3], long long *matches);
/* The peaks of a brute-force sweep's score landscape, picked on the device.  A matcher answers with one pose; in a
 * corridor or a symmetric room the landscape has a ridge or several maxima and a second pose is as good as the first.
 * These calls score the lattice a BruteForcePoseEnumerator hands out when `centre` is its latched base -- the matcher's
 * own offsets, pose bits made by the enumerator's additions, x fastest, then y, then theta; the initial-pose call 0 of a
 * match is not part of it: lattice index j is call j + 1 of a sweep -- and return its local maxima above two floors, best
 * first.  The rule, one text for host and device (csrc/bf_peaks.h):
 *  - key order: a beats b iff score a > score b, or the scores are equal and a < b (the pose handed out first, the
 *    matcher's own "first pose holding the maximum").  A NaN score is absent: it beats nothing and is never a peak.
 *  - window of i: |dx| <= radius[0], |dy| <= radius[1], |dtheta| <= radius[2] in lattice steps, clipped at the faces of
 *    the volume (theta does not wrap); 0 <= radius <= 32.  i is a peak iff its score is not NaN and nothing else in its
 *    window beats it.  Radius (0, 0, 0): every non-NaN point, i.e. the N best poses.
 *  - floors: with s_max the largest non-NaN score of the lattice, a peak is kept iff
 *    score >= min_score && score >= min_ratio * s_max.  An all-NaN lattice has no peaks.
 *  - result: kept peaks in descending score, ties by ascending index; *n_found = how many were kept, *n_written =
 *    min(*n_found, max_peaks) entries of peaks_out.  max_peaks = 0 counts only (peaks_out may be NULL).
 *  - bound: two peaks never lie in each other's window, so at most B = ceil(nx / (rx + 1)) ceil(ny / (ry + 1))
 *    ceil(nt / (rt + 1)) exist.  B > 8192 is SLAMHIP_ERR_INVALID: widen the radius or narrow the sweep.
 * Peaks are those of the canonical sums -- bit-equal to slamhip_score_poses on the same poses; the checked default mode's
 * tie check (slamhip_matcher_set_tie_check) is NOT applied.  The lone call scores the context's current scan; in the
 * batch, job k's init_pose is its centre and map and scan come per job as in slamhip_matcher_process_scan_batch, job k
 * equals the lone call on its inputs, K x (1 + nx ny nt) <= 2^24.  The jobs are scored in ONE shared launch where the
 * batched sweep's scoring kernel covers them (1-cell OOPE, one effective cell model, at most 4096 beams a job), else job
 * after job; three more launches, whatever n, K and the radius, pick the peaks of all jobs, and only the counts and the
 * written peaks cross the bus.
 *  - State: the enumerator and its latch, the enumerator streams, the observer and every counter of
 *    slamhip_matcher_stats are neither read nor written; the context's current scan stays what it was.  For the
 *    landscape of the next process_scan pass the base slamhip_matcher_bf_stream_info(m, -1, ...) reports, or the initial
 *    pose while none is latched.
 *  - Covered: point and window OOPEs, OCC / TBM / CREDIBILIST maps (through the probability plane where the sweep goes
 *    through it), SLAMHIP_SUM_TREE256, device pose trigonometry, at most 2^26 poses.  The GMapping OOPE, the beam-order
 *    sum and host or RAW_EXACT pose trigonometry: SLAMHIP_ERR_UNSUPPORTED.
 *  - SLAMHIP_ERR_INVALID: a matcher that is not brute force, a radius outside 0 ... 32, B > 8192, max_peaks outside
 *    0 ... 8192, min_ratio outside [0, 1], a NaN min_score, null arguments (shape_out may be NULL), a batch beyond 2^24
 *    poses.  Every refusal comes before anything is launched.
 * shape_out: (nx, ny, nt).  index: ix + nx (iy + ny it). */
typedef struct {
  double pose[3];
  double score;
  long long index;
} slamhip_bf_peak;
int slamhip_matcher_bf_peaks(slamhip_matcher *m, int map_id, const double centre[3], const int radius[3], double min_ratio,
                             double min_score, int max_peaks, slamhip_bf_peak *peaks_out, int *n_written, long long *n_found,
                             int shape_out[3]);
int slamhip_matcher_bf_peaks_batch(slamhip_matcher *m, int n_jobs, const slamhip_match_job *jobs, const int radius[3],
                                   double min_ratio, double min_score, int max_peaks,
                                   slamhip_bf_peak *peaks_out /* n_jobs x max_peaks */, int *n_written /* n_jobs */,
                                   long long *n_found /* n_jobs */);
/* the last peaks call that got as far as launching: the kernels it launched, counted where they are launched (pose and
 * scoring kernels included; not among them: the one-off derivation of a TBM / CREDIBILIST map's probability plane, which
 * the first scoring call of any kind over such a map makes), its bound B, and whether its jobs were scored in the shared
 * launch.  A refused call leaves all three as they were.  Zeros before the first. */
int slamhip_matcher_bf_peaks_stats(slamhip_matcher *m, long long *launches, long long *survivors_bound, int *on_shared_launch);
/* the rule on the host, no GPU: the peaks of scores[ix + nx (iy + ny it)]; index_out / score_out: max_peaks entries */
int slamhip_bf_peaks_host(const double *scores, int nx, int ny, int nt, const int radius[3], double min_ratio, double min_score,
                          int max_peaks, long long *index_out, double *score_out, int *n_written, long long *n_found);
/* counters of the last process_scan: scorer calls the reference would have made
 * (= on_scan_test events), poses actually evaluated on the GPU, launches */
int slamhip_matcher_stats(slamhip_matcher *m, long long *scorer_calls, long long *poses_evaluated,
                          long long *launches);

/* device chain only (zeros otherwise), last process_scan: kernels launched (super-steps + run-ahead launches that
 * found the chain finished) and super-steps the checked default mode scored a second time in beam order because
 * a comparison on the path was too close for the canonical tree sum to settle */
int slamhip_matcher_chain_stats(slamhip_matcher *m, long long *kernels_launched, long long *steps_rescored);
/* last process_scan / batch: scorer calls (of slamhip_matcher_stats' count) that were reported in closed form instead
 * of being scored -- the tail of a hill-climbing match whose candidates have all become the best pose itself
 * (SLAMHIP_OPT_INERT_TAIL; hill_climbing_scan_matcher.h:83-101).  0 on every other path. */
int slamhip_matcher_tail_stats(slamhip_matcher *m, long long *calls_closed_form);

/* host-side time split of the last process_scan in microseconds: building the speculation DAG,
 * staging poses, launch + wait for scores, replay of the accept chain */
int slamhip_matcher_timing(slamhip_matcher *m, double *build_us, double *stage_us, double *score_us,
                           double *replay_us);

/* ---------------------------------------------------------------- particle filter (K4/K5)
 * ParticleFilter::normalize_weights / UniformResamling (src/core/particle_filter.h:34-66,108-121)
 * in the reference's summation order (host; N <= a few hundred).  Sharded runs all-gather the raw
 * weights first (RCCL) and call these on every rank so indices are bit-identical. */
int slamhip_pf_normalize(int n, double *weights);
int slamhip_pf_resampling_is_required(int n, const double *weights, int *required);
int slamhip_pf_resample(int n, const double *weights, uint32_t seed, unsigned *out_idx);
int slamhip_pf_heaviest(int n, const double *weights, int *index);

/* ---------------------------------------------------------------- GMapping particle filter
 * Replaces LaserScanGridWorld::handle_sensor_data of GmappingParticleFilter
 * (src/slams/gmapping/gmapping_particle_filter.h:45-50; per particle GmappingWorld::update_robot_pose
 * / handle_observation, src/slams/gmapping/gmapping_world.h:57-101) for the likelihood part of
 * the step: odometry, matching gate, pose noise, HC(6, 0.1, 0.1) scan matching of all particles in
 * lock-step on the GPU, weight update, normalisation, N_eff test, multinomial resampling with
 * duplicated particles and master hand-over.  The map update inside the step (gmapping_world.h:93-97) comes in
 * two forms: slamhip_gmapping_set_map_update (the reference's ONE shared map, updated particle after particle)
 * and slamhip_gmapping_enable_particle_maps (a copy-on-write map per particle, one batched update per step).
 *
 * A filter object holds the particles [first, first + count) of n_total (one object per GPU when
 * particles are sharded).  Sharded step:
 *   1. every rank:  slamhip_gmapping_predict_match(...)            -> raw weights of its shard
 *   2. caller:      all-gather the raw weights (n_total doubles)      [the one collective, RCCL]
 *   3. every rank:  slamhip_gmapping_plan_resample(all weights)    -> identical decision + indices
 *   4. if required: slamhip_gmapping_export -> all-gather n_total records -> slamhip_gmapping_import
 * slamhip_gmapping_step does 1-4 for an unsharded filter. */
typedef struct slamhip_gmapping slamhip_gmapping;
typedef struct {
  /* GMappingParams (src/slams/gmapping/gmapping_world.h:16-34, defaults init_gmapping.h:15-34) */
  double mean_sample_xy, sigma_sample_xy, mean_sample_th, sigma_sample_th;
  double min_sm_lim_xy, max_sm_lim_xy, min_sm_lim_th, max_sm_lim_th;
  /* HillClimbingScanMatcher(6, 0.1, 0.1) hard-wired in init_gmapping.h:58-60 */
  unsigned hc_failed_rounds_limit;
  double hc_translation, hc_rotation;
  /* WeightedMeanPointProbabilitySPE(oope, EvenSPW, skip_rate, max_range), init_scan_matching.h:94-109 */
  unsigned sp_skip_rate;
  double sp_max_usable_range;
  /* GmappingOccupancyObservationPE(fullness_th, window), init_gmapping.h:36-45 */
  double oope_fullness_th;
  int oope_window;
  int pose_trig; /* SLAMHIP_POSE_TRIG_* */
} slamhip_gmapping_params;

/* seeds: one per LOCAL particle = what std::random_device hands the GmappingWorld ctor
 * (gmapping_world.h:51).  ctx may be NULL for host-only bookkeeping (steps 3-4). */
int slamhip_gmapping_create(slamhip_ctx *ctx, const slamhip_gmapping_params *prm, int n_total,
                            int first, int count, const uint32_t *seeds, slamhip_gmapping **out);
int slamhip_gmapping_destroy(slamhip_gmapping *g);
/* raw scan (unfiltered); raw_weights_out: count doubles (weight * scan probability, unnormalised) */
int slamhip_gmapping_predict_match(slamhip_gmapping *g, int map_id, int n_raw, const double *range,
                                   const double *angle, const int *is_occ, const double odom_delta[3],
                                   double *raw_weights_out);
/* ParticleFilter::normalize_weights + the try_resample gates (gmapping_particle_filter.h:88-99,
 * particle_filter.h:34-43) + UniformResamling::resample (:45-66) over ALL n_total weights;
 * idx_out (n_total) is written when *required becomes 1 */
int slamhip_gmapping_plan_resample(slamhip_gmapping *g, const double *all_raw_weights,
                                   uint32_t resample_seed, int *required, unsigned *idx_out);
size_t slamhip_gmapping_blob_size(void);
int slamhip_gmapping_export(slamhip_gmapping *g, void *blobs_out /* count records */);
/* ParticleFilter::try_resample body (particle_filter.h:88-105) + ensure_master_exists */
int slamhip_gmapping_import(slamhip_gmapping *g, const void *all_blobs /* n_total records */,
                            const unsigned *idx /* n_total */);
int slamhip_gmapping_step(slamhip_gmapping *g, int map_id, int n_raw, const double *range,
                          const double *angle, const int *is_occ, const double odom_delta[3],
                          uint32_t resample_seed, int *resampled, unsigned *idx_out);
int slamhip_gmapping_set(slamhip_gmapping *g, const double *poses, const double *weights);
/* cfg != NULL: every matching particle appends its scan to the map (scan adder of init_gmapping,
 * init_occupancy_mapping.h:82-92; rule and scan_quality are overridden: GmappingBaseCell, 1.0) right
 * after its match, BEFORE the next particle matches -- the reference's particles share one map
 * object (Q20), which makes this step sequential and unshardable.  NULL switches it off. */
int slamhip_gmapping_set_map_update(slamhip_gmapping *g, const slamhip_scan_adder_cfg *cfg);
/* Per-particle maps: every particle gets its OWN map, a copy-on-write copy of the bound
 * GMAPPING window `map_id`, held as 128x128-cell tiles in a device pool with the sharing semantics of
 * UnboundedLazyTiledGridMap (src/core/maps/lazy_tiled_grid_map.h:18-187: a map copy copies tile
 * references :40-45, untouched area is one shared unknown tile :28-34, a write clones a shared tile
 * first :57-71).  This is what GmappingWorld's per-particle map member is for
 * (gmapping_world.h:36-55); the reference revision never separates them (Q20), so the mode has no
 * reference run -- parity is against the oracle with per-particle maps.  The step then keeps the
 * lock-step matching and appends the scans of all matched particles in ONE batched K6; a resampling
 * copies tile tables (particle_filter.h:92-96).  extent_tiles: side of the initial virtual extent in
 * tiles; it grows by whole tiles when a scan reaches beyond it, like the reference's unbounded maps
 * (lazy_tiled_grid_map.h:128-187; cells outside read as unknown); pool_tiles: capacity (768 KiB each).
 * A shard [first, first+count) of the filter holds the maps of its own particles; when a resampling
 * draws a particle that lives on another rank its map travels as one exported buffer (below). */
int slamhip_gmapping_enable_particle_maps(slamhip_gmapping *g, int map_id, const slamhip_scan_adder_cfg *cfg,
                                          int extent_tiles, int pool_tiles);
/* external window of one particle's map: payload3 = (prob_occ, obstacle x, obstacle y) per cell,
 * aux2 = (hits, tries) per cell; either may be NULL */
int slamhip_gmapping_particle_map_download(slamhip_gmapping *g, int particle, int x0, int y0, int w, int h,
                                           double *payload3, double *aux2);
/* The same EXTERNAL window of one particle's map as slamhip_map_render's bytes (format as there; the cells are
 * GMAPPING cells), out: w * h bytes: the map observers' cell loops (occupancy_grid_publisher.h:40-46,
 * map_dumpers.h:78-87) over a particle's LazyTiledGridMap, 1 byte per cell to the host instead of the download's 40.
 * Cells outside the pool's extent read as the never-observed cell: -1 / 127.  Only prob_occ is read; the update
 * counters do not enter.  SLAMHIP_ERR_INVALID: a filter without particle maps, an unknown particle, null out, unknown
 * format, an empty window. */
int slamhip_gmapping_particle_map_render(slamhip_gmapping *g, int particle, int format, int x0, int y0, int w, int h,
                                         void *out);
/* Laser scans ray-cast from the particles' OWN maps ("scan generation" above: semantics, status bytes, `variant` and
 * `flags` are slamhip_map_generate_scans'): job k = n_angles beams from pose poses_xyt[3k..3k+2] over the map of LOCAL
 * particle particles[k] (indices as slamhip_gmapping_particle_map_download takes them; a particle may be named by
 * several jobs), all jobs in ONE launch over the tile pool -- what a particle should see from its map, without the
 * 40-byte-per-cell download and dense re-upload.  range_out[n_jobs][n_angles] doubles, status_out one byte per beam in
 * the same order.  The cells are GMAPPING cells: double(map[cell]) is prob_occ; a cell outside the pool's extent reads
 * as the never-observed cell (-1), so does the shared unknown tile.  Queued on the context's stream behind every queued
 * pool operation (clones, table patches, appends); writes nothing to the pool; one copy up, one back.  While
 * slamhip_profile_enable is on, the kernel's time is added to kernel_ms_total.  SLAMHIP_ERR_INVALID, before anything is
 * queued: a filter without particle maps, a particle out of range, unknown flags, and everything
 * slamhip_map_generate_scans refuses for a dense map of the pool's scale.  n_jobs == 0 or n_angles == 0: OK, nothing
 * happens. */
int slamhip_gmapping_particle_generate_scans(slamhip_gmapping *g, int variant, int flags, int n_jobs, const int *particles,
                                             const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                                             double occ_threshold, double *range_out, unsigned char *status_out);
/* Pose sets scored over the particles' OWN maps: job k = n_poses poses under one scan over the map of LOCAL particle
 * `particle` (indices as slamhip_gmapping_particle_map_download takes them; a particle may be named by several jobs;
 * scan_slot as in slamhip_score_job: a scan of slamhip_scan_store on the filter's context, or -1 for its current scan),
 * all jobs through ONE scoring launch over the tile pool and ONE launch that carries each job's run cache from pose to
 * pose -- a heat map over the heaviest particle's map, likelihoods of poses sampled around every particle's pose, "which
 * particle's map explains this scan", without the 40-byte-per-cell download and dense re-upload.  scores_out: the jobs'
 * scores one job after the other, sum of n_poses doubles.
 * Configuration: cfg->oope must be SLAMHIP_OOPE_GMAPPING (the pool holds GMAPPING cells); gm_window 0..4, any
 * gm_fullness_th; sum_order SLAMHIP_SUM_TREE256; pose_trig SLAMHIP_POSE_TRIG_DEVICE or _HOST.
 * Value: job k's scores are bit-equal to slamhip_gmapping_particle_map_download of a window that covers the pool's
 * extent, that window bound and uploaded as a dense SLAMHIP_CELL_GMAPPING map, slamhip_gm_cache_reset,
 * slamhip_scan_select(scan_slot) and slamhip_score_poses(that map, cfg, the job's poses) -- whatever the other jobs are,
 * whichever kernel form runs and however poses are dealt to workgroups.  NaN where the scan's weights add up to 0.  A
 * cell outside the pool's extent and the shared unknown tile both read as the never-observed cell, as in the render and
 * scan-generation calls above.
 * Run cache: GmappingOccupancyObservationPE's _cached_coord / _cached_prob (gmapping_occupancy_observation_pe.h:21-24,
 * 36-37) starts EMPTY for every job and is carried from pose to pose within the job, in the order given: a job is one
 * estimator object scoring its list.  The context's own cache (slamhip_gm_cache_get) and its current scan are what
 * they were before the call.
 * Neighbourhood masks: the tiles' masks are used only when the pool's masks are valid for cfg->gm_fullness_th and
 * gm_window == 1 (the filter's own matching configuration); the call never re-derives them for another threshold --
 * such a call reads the nine cells.
 * Queued on the context's stream behind every queued pool operation (clones, table patches, appends); writes nothing to
 * the pool; returns with scores_out filled.  A call with at least one pose makes exactly TWO launches, scoring and
 * carry, whatever the number of jobs, and ONE host-to-device copy (a pinned arena: job table, block table, poses and,
 * under SLAMHIP_POSE_TRIG_HOST, their sin / cos).  n_jobs == 0 and jobs with n_poses == 0 are legal and launch nothing;
 * such a job's particle and slot are not looked at.  While slamhip_profile_enable is on, both kernels' time is added
 * to kernel_ms_total.
 * Errors are found before anything is staged or queued and leave scores_out, the stats below, the current scan and
 * the cache untouched.  SLAMHIP_ERR_INVALID: null arguments, a filter without particle maps, a particle out of range,
 * a slot out of range, another OOPE, SLAMHIP_SUM_SEQUENTIAL or SLAMHIP_POSE_TRIG_RAW_EXACT (not built: the exact
 * modes stay with the filter's own path), a scan above 2048 points ("the GMapping kernel holds at most 2048 filtered
 * beams per scan").  SLAMHIP_ERR_STATE: an empty slot, slot -1 without a current scan. */
typedef struct {
  int particle;            /* LOCAL particle index; may repeat over jobs */
  int scan_slot;           /* 0..4095: a scan of slamhip_scan_store on the filter's context; -1: its current scan */
  int n_poses;             /* >= 0 */
  const double *poses_xyt; /* n_poses x (x, y, theta), host */
} slamhip_particle_score_job;
int slamhip_gmapping_particle_score_poses(slamhip_gmapping *g, const slamhip_spe_cfg *cfg, int n_jobs,
                                          const slamhip_particle_score_job *jobs,
                                          double *scores_out /* sum of n_poses, job after job */);
/* Of the last slamhip_gmapping_particle_score_poses that was not refused: jobs with poses, poses, kernels launched
 * (2, or 0 for a call without poses), and the poses whose first run took the carried value instead of its fresh one. */
int slamhip_gmapping_particle_score_stats(slamhip_gmapping *g, int *jobs_scored, long long *poses_scored,
                                          int *launches, long long *poses_carried);
/* The append half of GmappingWorld::handle_observation (gmapping_world.h:93-97) for a set of local
 * particles at once: the raw scan is appended to the map of particle particles[k] from poses3[3k..3k+2] --
 * ONE batched K6 over all (particle, beam) pairs, copy-on-write first.  The filter step does this itself for
 * the particles that matched; this entry point is for callers that place scans from their own poses. */
int slamhip_gmapping_particle_maps_append(slamhip_gmapping *g, int n_jobs, const int *particles,
                                          const double *poses3, int n_raw, const double *range,
                                          const double *angle, const int *is_occ, long long *n_updates);
int slamhip_gmapping_particle_map_stats(slamhip_gmapping *g, long long *tiles_in_use, long long *tiles_shared,
                                        long long *bytes, long long *cow_copies, long long *cell_updates);
/* Migration of a particle's map to another rank (the "moving a duplicated particle to another GPU"
 * step of SURVEY 8e).  Export: every tile the LOCAL particle references (except the unknown tile) into a
 * host buffer: int64 n_tiles, per tile four int32 (x, y of its first cell in external coordinates -- so
 * that pools whose extents grew differently still agree --, ordinal of the common ancestor tile it
 * still is or -1, 0), then per non-ancestor tile 16384 x 4 payload and 16384 x 2 counter doubles.
 * The receiving pool grows first if the map reaches beyond it.  Exports must be taken before any rank
 * imports. */
int slamhip_gmapping_particle_map_export_size(slamhip_gmapping *g, int particle, size_t *bytes);
int slamhip_gmapping_particle_map_export(slamhip_gmapping *g, int particle, void *host_buf, size_t cap);
/* slamhip_gmapping_import for a filter with per-particle maps: new local particle l takes the map of
 * old particle idx[first + l] -- a table copy when that one is local, otherwise the exported buffer
 * remote_bufs[k] with remote_src[k] == idx[first + l] (GLOBAL particle index; a source used by several
 * new particles is listed and imported once, its tiles are then shared copy-on-write). */
int slamhip_gmapping_import_maps(slamhip_gmapping *g, const void *all_blobs, const unsigned *idx, int n_remote,
                                 const int *remote_src, const void *const *remote_bufs);
int slamhip_gmapping_get(slamhip_gmapping *g, double *poses, double *weights, int *is_master);

/* ---------------------------------------------------------------- sharding over GPUs (RCCL over xGMI)
 * What gets distributed is ParticleFilter's particle loop (src/core/particle_filter.h:108-112 over
 * GmappingWorld::handle_sensor_data) -- one shard [first, first + count) of the particles per GPU, one
 * process (or thread) per GPU, one context each -- and what has to be collected is what
 * normalize_weights / UniformResamling read: ALL raw weights, in particle order (:34-66).  The one
 * collective of a step is therefore an all-gather of n_total doubles; an all-reduce of (sum w, sum w^2)
 * would be smaller but adds in another order than the reference does, and resampling indices must stay
 * bit-exact.  RCCL is loaded when the first of these functions is called (librccl.so is not a link
 * dependency of libslamhip.so).
 *   rank 0:      slamhip_shard_unique_id(id)          -> hand the 128 bytes to the other ranks (MPI, a
 *                                                        file, a socket: whatever started the processes)
 *   every rank:  slamhip_shard_init(ctx, rank, world, id)
 *   per scan:    slamhip_gmapping_step_sharded(...)   = match_begin, the carry exchange, match_finish,
 *                                                        all-gather of the raw weights, plan_resample and,
 *                                                        when a resampling happens, all-gather of the
 *                                                        particle records + import
 *
 * slamhip_gmapping_step_sharded needs ONE collective per step in the common case: the carry records travel together
 * with the raw weights the particles will have if no cache hand-over needs repair, and whether one does is read off
 * the records by every rank alike (no flags exchanged).
 *
 * A caller with its own means of moving bytes between the ranks (MPI, shared memory, a test harness that runs the
 * ranks as threads of one process) joins a group with slamhip_shard_attach instead of slamhip_shard_init and hands in
 * a slamhip_shard_transport; everything above the transport -- slamhip_shard_allgather's padding,
 * slamhip_gmapping_step_sharded -- is the same code either way (tests/native/loopback_transport.cpp is such a
 * transport: it is how the sharded step runs with world > 1 on the one GPU of a test box, RCCL admitting one rank
 * per device). */
#define SLAMHIP_SHARD_ID_BYTES 128
int slamhip_shard_unique_id(void *id_out);
int slamhip_shard_init(slamhip_ctx *ctx, int rank, int world, const void *id);
int slamhip_shard_destroy(slamhip_ctx *ctx);
int slamhip_shard_info(slamhip_ctx *ctx, int *rank, int *world);
/* all-gather of per-rank blocks: rank r contributes counts[r] elements of elem_bytes bytes (host memory,
 * `local`); `all_out` (host) receives the blocks in rank order.  Blocks are padded to the largest one on
 * the wire (100 particles on 8 GPUs are 13 x 4 + 12 x 4). */
int slamhip_shard_allgather(slamhip_ctx *ctx, const void *local, const int *counts, int elem_bytes,
                            void *all_out);
/* bytes moved through RCCL and collectives issued since slamhip_shard_init */
int slamhip_shard_stats(slamhip_ctx *ctx, long long *collectives, long long *bytes);
/* Point to point, all ranks together: this rank sends n_send blocks and receives n_recv.  Buffers are DEVICE memory of
 * the context's GPU; messages between one pair of ranks are matched in the order they are listed on both sides.  Over
 * RCCL this is one ncclGroupStart .. ncclSend / ncclRecv .. ncclGroupEnd on the context's stream (xGMI is point to
 * point: a pair's bytes travel on the link between the two GPUs), awaited before the call returns.  It is what carries a
 * resampled particle's map to the rank that drew it (particle_filter.h:88-103: `*new_particle = *sampled` copies
 * the whole world; lazy_tiled_grid_map.h:40-71: tile by tile). */
typedef struct {
  int peer;
  void *buf;
  size_t bytes;
} slamhip_shard_msg;
int slamhip_shard_exchange(slamhip_ctx *ctx, int n_send, const slamhip_shard_msg *send, int n_recv,
                           const slamhip_shard_msg *recv);
int slamhip_shard_p2p_stats(slamhip_ctx *ctx, long long *exchanges, long long *bytes_sent);
/* Every wait on a collective of the built-in (RCCL) transport is bounded: slamhip_shard_allgather / _exchange poll the
 * stream until the deadline (default 30 s; ms <= 0 restores it) and then return SLAMHIP_ERR_TIMEOUT -- a peer that
 * died INSIDE a collective, which no status word can report.  The communicator is aborted (ncclCommAbort) and the
 * group is broken from then on: every later collective of this context fails at once with SLAMHIP_ERR_STATE, so a
 * sharded step in flight is abandoned on every survivor within the deadline; slamhip_shard_destroy + a fresh
 * slamhip_shard_init among the survivors start over.  (An attached transport bounds its own waits and reports
 * through its return code.) */
int slamhip_shard_set_timeout(slamhip_ctx *ctx, int ms);
/* A transport of the caller's: allgather moves equal blocks of host memory (every rank's block_bytes from send_host
 * into recv_host, world x block_bytes in rank order), exchange has the contract of slamhip_shard_exchange (device
 * buffers; the context's stream is idle when it is called), destroy (may be NULL) runs when the context leaves the
 * group.  Each returns 0 on success.  The table is copied. */
typedef struct {
  void *user;
  int (*allgather)(void *user, const void *send_host, size_t block_bytes, void *recv_host);
  int (*exchange)(void *user, int n_send, const slamhip_shard_msg *send, int n_recv, const slamhip_shard_msg *recv);
  void (*destroy)(void *user);
} slamhip_shard_transport;
int slamhip_shard_attach(slamhip_ctx *ctx, int rank, int world, const slamhip_shard_transport *t);

/* A step in phases, for callers that bring their own collective: match_begin = odometry, gate, pose noise
 * and the lock-step matching of the local shard; match_finish = poses, weights (and the batched map
 * update of per-particle maps); slamhip_gmapping_predict_match is begin + finish.
 * Between them, sharded steps repair the ONE OOPE cache the reference's particles hand from one to the
 * next (gmapping_occupancy_observation_pe.h:21-24,36-37,43-44): every shard starts its
 * first job without a carry (slamhip_gmapping_set_shard_chain), publishes a slamhip_carry_record, and
 * checks its first job against the final cache entry of the shard before it -- re-matching on a hit --
 * until no record changes any more (at most `world` rounds; none in practice). */
typedef struct {
  int has_active;                 /* some particle of the shard matched in this step */
  int first_cx, first_cy;         /* end-point cell of the first beam of its first scored pose ... */
  double first_v0;                /* ... and the fresh value of that beam */
  int carry_cx, carry_cy;         /* the cache entry the shard's last job ended with */
  double carry_prob;
} slamhip_carry_record;
int slamhip_gmapping_set_shard_chain(slamhip_gmapping *g, int on);
int slamhip_gmapping_match_begin(slamhip_gmapping *g, int map_id, int n_raw, const double *range,
                                 const double *angle, const int *is_occ, const double odom_delta[3]);
int slamhip_gmapping_carry_record(slamhip_gmapping *g, slamhip_carry_record *rec);
int slamhip_gmapping_carry_fix(slamhip_gmapping *g, const slamhip_carry_record *all, int world, int rank,
                               int *changed);
int slamhip_gmapping_carry_commit(slamhip_gmapping *g, const slamhip_carry_record *all, int world);
int slamhip_gmapping_match_finish(slamhip_gmapping *g, double *raw_weights_out);
/* One scan on a shard, collectives included (the filter's context has joined a group: slamhip_shard_init or
 * slamhip_shard_attach).  resampled / idx_out as in slamhip_gmapping_step; idx_out holds n_total indices.
 * Filters with per-particle maps (slamhip_gmapping_enable_particle_maps) are covered: when a resampling draws a
 * particle that lives on another rank, its map travels inside this call -- every rank reads the same migration plan
 * off the resampling indices; two small all-gathers carry the sizes and the maps' headers (tile positions, ancestor
 * ordinals), ONE slamhip_shard_exchange carries the tile contents device to device (RCCL send / recv), then
 * slamhip_gmapping_import_maps' work is done from the received buffers (particle_filter.h:88-103: the reference's
 * resampling copies whole worlds; lazy_tiled_grid_map.h:40-71: maps copy tile by tile).
 * Errors: a rank that fails inside a step says so in the status word of the step's next collective, and EVERY rank
 * returns from that step with an error (the failing one with its own code, the others with SLAMHIP_ERR_STATE)
 * instead of waiting for it; a failure behind a step's last collective is announced at the start of the next
 * step.  A filter whose step was abandoned is usable again (slamhip_gmapping_match_abort does the same for callers
 * that drive the phases themselves): the particles keep the odometry and pose noise the step had applied. */
int slamhip_gmapping_step_sharded(slamhip_gmapping *g, int map_id, int n_raw, const double *range,
                                  const double *angle, const int *is_occ, const double odom_delta[3],
                                  uint32_t resample_seed, int *resampled, unsigned *idx_out);
int slamhip_gmapping_match_abort(slamhip_gmapping *g);
/* maps this shard received from other ranks and tile bytes it sent, since the filter was created */
int slamhip_gmapping_migration_stats(slamhip_gmapping *g, long long *maps_received, long long *tile_bytes_sent);
int slamhip_gmapping_stats(slamhip_gmapping *g, long long *scorer_calls, long long *poses_evaluated,
                           long long *launches, long long *carry_reruns);

#ifdef __cplusplus
}
#endif
#endif /* SLAMHIP_H */
