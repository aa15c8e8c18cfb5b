/* sps_hip.h -- C ABI of libsps_hip.so: the MI355X (gfx950) native implementation of the
 * SPS per-scan sparse-convnet hot path.
 *
 * The reference (ibrahimhroob/SPS) has no native code of its own; the native boundary it
 * crosses on this path is MinkowskiEngine's pybind11 module (MinkowskiEngineBackend._C:
 * CoordinateMapManager, ConvolutionForwardGPU, ...), reached from the Python call sites
 * cited next to each entry point below.  This header is what a maintainer binds INSTEAD of
 * MinkowskiEngine for that path (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *   - every function returns SPS_OK (0) or a negative error code; the message for the last
 *     error on the calling thread is available from sps_last_error();
 *   - no exceptions and no torch types cross the boundary: plain pointers and sizes;
 *   - pointers named *_dev are DEVICE pointers owned by the caller (torch tensors'
 *     data_ptr()); *_host are host pointers; the library owns only what lives inside ctx
 *     (arena, hash tables, weights);
 *   - one ctx per (process, device); a ctx is not thread-safe; all work is ordered on the
 *     hipStream_t passed as `stream` (void*, NULL = the default stream) and functions do
 *     not synchronise with the host unless their comment says so.
 */
#ifndef SPS_HIP_H
#define SPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPS_OK 0
#define SPS_ERR_INVALID (-1) /* bad argument / state                              */
#define SPS_ERR_HIP (-2)     /* a HIP runtime call failed                        */
#define SPS_ERR_NOMEM (-3)   /* device allocation failed / compact arena overflow */
#define SPS_ERR_RANGE (-4)   /* a coordinate does not fit the 64-bit voxel key   */
#define SPS_ERR_NOWEIGHTS (-5)
#define SPS_ERR_ITEMCAP (-6) /* sps_radius_item: the caller's item buffer is too small; sps_radius_crop: crop capacity */

#define SPS_NUM_LEVELS 5 /* tensor strides 1,2,4,8,16 (minkunet.py:161-219) */

/* Voxel-key range (sps_amd/csrc/sps_hip.hip packs (b,x,y,z,t) into 64 bits):
 * x,y,z in [-131072, 131071] voxels, t in [-16, 15], b in [0, 30]. */
#define SPS_COORD_MIN (-131072)
#define SPS_COORD_MAX (131071)
#define SPS_T_MIN (-16)
#define SPS_T_MAX (15)
#define SPS_BATCH_MAX (30)
#define SPS_MAX_POINTS (1 << 23) /* rows per forward / submap call (32-bit byte offsets into [rows,96] f32) */

typedef struct sps_ctx sps_ctx;

const char *sps_last_error(void);
int sps_version(void);

/* ---- context ------------------------------------------------------------------------ */
/* Replaces the per-forward ME coordinate manager + the module's .cuda() placement
 * (reference scripts/predict.py:59, src/sps/datasets/util.py:40). */
int sps_ctx_create(int device, sps_ctx **out);
int sps_ctx_destroy(sps_ctx *ctx);
/* Pre-size the arena for clouds of up to max_points rows (optional: sps_forward grows it
 * on demand, which synchronises the device). */
int sps_reserve(sps_ctx *ctx, int64_t max_points);
/* Arena sizing.  By default every tensor stride ("level" l = 0..4, stride 2^l) can hold as many voxels as there are
 * points: no input can overflow, at ~6.9 KB of device memory per point.  LiDAR clouds thin out quickly with the stride
 * (V_l / V_0 ~ 0.39 / 0.14 / 0.05 / 0.015 at 0.1 m), so a streaming caller may give level l only frac[l] * max_points rows
 * (frac[0] is ignored: level 0 always holds every point; blocks get half the rows' capacity): ~2.2 KB per point with
 * {1, 0.6, 0.3, 0.15, 0.08}.  A forward whose cloud needs more is ABORTED on the device (its scores are NaN) and the next
 * synchronising call (sps_check, sps_metrics) returns SPS_ERR_NOMEM after switching the context back to full-size
 * arenas; the caller re-issues it.  frac = NULL restores the default.  Takes effect at the next reserve / forward
 * (re-allocation: synchronises).  sps_arena_bytes: device bytes the context's arena holds. */
int sps_ctx_set_level_fractions(sps_ctx *ctx, const float *frac);
int64_t sps_arena_bytes(sps_ctx *ctx);
/* Inference-only context (streaming callers: sps_amd.engine.ScanEngine).  The one-column-tile 3x3x3x3 layers of levels 0 and 1
 * run on the map's RULEBOOK (per 64-row supertile and offset the compacted (output row, input row) pairs; the counterpart of
 * ME's kernel map, in / out index lists per offset), which k_maps builds next to the output-stationary neighbour table.
 * on != 0: at those levels the rulebook takes the place AND the memory of the neighbour table, which is then neither written
 * nor kept (17 MB less to store per config-2 scan, 324 B per row less arena): sps_get_nbr fails there, sps_get_map_pairs
 * counts from the rulebook, and sps_train_forward switches the context back (re-allocation).  Takes effect at the next
 * reserve / forward (re-allocation: synchronises). */
int sps_ctx_set_inference_only(sps_ctx *ctx, int on);
/* How the context's forwards are scheduled -- a hint for the launch geometry, never for the results (bit-identical either way).
 * on == 0 (default): one forward after another (a plain `model(batch)` loop, the online filter: sps_node.callback handles one scan
 * at a time, sps_node.py:88-176): the coarse levels, which hold few tiles, run one column tile per wave -- the shortest chain
 * (serial forward 366 -> 359 us at config 2).  on != 0: forwards of several contexts are in flight beside each other
 * (sps_amd.engine.ScanEngine with more than one pipeline; no reference counterpart: predict.py:64-67 is one Trainer loop): two
 * column tiles per wave -- half the gathers for the same MFMAs, +1.3-1.8 % scans/s pipelined.  Takes effect at the next forward. */
int sps_ctx_set_pipelined(sps_ctx *ctx, int on);

/* ---- weights ------------------------------------------------------------------------
 * Replaces nn.Module.load_state_dict on CustomMinkUNet (reference scripts/predict.py:56-58,
 * src/sps/datasets/util.py:33-39).  The blob is the concatenation of the tensors listed by
 * sps_weights_tensor_info in index order; names are the reference state_dict keys without
 * the "model.MinkUNet." prefix, e.g. "block2.0.conv1.kernel" [81,8,16],
 * "block2.0.downsample.0.kernel" [8,16], "bn0.bn.running_var" [8], "final.bias" [1]. */
int sps_weights_num_tensors(void);
int sps_weights_tensor_info(int idx, char *name, int name_cap, int64_t *offset, int64_t *numel);
int64_t sps_weights_numel(void);
/* Copies the blob to the device and derives the folded BatchNorm scale/shift
 * (eval mode, eps = 1e-5).  Blocking copies into fresh allocations (= sps_weights_create + sps_ctx_set_weights). */
int sps_weights_load(sps_ctx *ctx, const float *blob_host, int64_t numel);
/* A device-resident weight set that several contexts of one device share (a pipelined loop runs one context per
 * stream: the module's .cuda() happens once, reference scripts/predict.py:59, not once per stream).
 * sps_weights_create uploads (blocking copies, no device-wide synchronise); sps_ctx_set_weights attaches it to a
 * context in O(1) without any synchronisation -- forwards issued afterwards use it, forwards already issued keep
 * reading the previous set, which stays alive until its last user lets go; sps_weights_destroy drops the caller's
 * reference.  out_channels as in sps_weights_load_head below. */
typedef struct sps_weights_handle sps_weights_handle;
int sps_weights_create(int device, const float *blob_host, int64_t numel, int out_channels, sps_weights_handle **out);
int sps_weights_destroy(sps_weights_handle *w);
int sps_ctx_set_weights(sps_ctx *ctx, sps_weights_handle *w);

/* ---- forward ------------------------------------------------------------------------
 * Replaces SPSModel.forward (reference src/sps/models/models.py:20-30): quantise by
 * [1,vs,vs,vs,1] in f32, floor, unique voxels + inverse map, CustomMinkUNet (33 sparse
 * convs + eval BN + ReLU + residual + concat), slice back to points, sigmoid.
 *   coords_dev : float32 rows (b,x,y,z,t,...) with row stride `ld` floats (ld >= 5)
 *   scores_dev : float32 [n]
 * Rows whose voxel does not fit the key range get score NaN and the call that next
 * synchronises (sps_metrics / sps_check) reports SPS_ERR_RANGE.
 * NOT capturable into a HIP graph: the single-pass ranking kernels tell the forwards of a context apart by a generation
 * number that is a KERNEL ARGUMENT (host counter); a replayed graph would carry a frozen generation and match the previous
 * replay's aggregates without waiting for them.  Every forward must be issued through these entry points. */
int sps_forward(sps_ctx *ctx, const float *coords_dev, int64_t ld, int64_t n, float voxel_size,
                float *scores_dev, void *stream);
/* Synchronises `stream` and returns SPS_ERR_RANGE if any forward since the last check
 * met an unrepresentable coordinate. */
int sps_check(sps_ctx *ctx, void *stream);

/* Forward + metric sums in one call = one scan of SPSNet.predict_step (reference models.py:84-105): `batch_dev` rows
 * are (b,x,y,z,t,label,...) as BacchusModule.collate_fn builds them (ld >= 6); scores_dev [n] as sps_forward,
 * out_dev [n_batches][8] doubles as sps_metrics_dev.  The sums are accumulated by the forward's last kernel while it
 * produces the scores (no separate fill / metrics launches, no second pass over the scores). */
int sps_forward_metrics(sps_ctx *ctx, const float *batch_dev, int64_t ld, int64_t n, float voxel_size, float eps,
                        int n_batches, float *scores_dev, double *out_dev, void *stream);

/* ---- baseline heads on the same backbone ------------------------------
 * The two baselines the reference ships run the SAME CustomMinkUNet14 wiring:
 *   4DMOS  : MOS4DNet.forward  (reference c_ws/src/mos4d/scripts/mos4d.py:11-32) --
 *            CustomMinkUNet(in_channels=1, out_channels=3), constant 0.5 feature, t = scan index of
 *            a 10-scan buffer, voxel 0.2 m, returns the raw logits of column 2;
 *   MapMOS : MapMOSNet.forward (reference c_ws/src/mapmos/scripts/mapmos.py:59-83) --
 *            out_channels=1, a per-point feature (1 + normalised index) whose per-voxel mean
 *            feeds conv0 (ME UNWEIGHTED_AVERAGE), t in {0,-1}, returns raw logits.
 * sps_head_* describe the weight blob of a k-channel `final` (spec as sps_weights_*, with
 * "final.kernel" [8,k] and "final.bias" [k]); sps_weights_load_head(…, k) loads it (k = 1 is
 * sps_weights_load).  sps_forward_head:
 *   feats_dev : float32 [n] per-point input feature, or NULL for the constant 0.5
 *   t_base    : integer subtracted from floor(t) before hashing (the network is shift-invariant
 *               along t; lets a long-running scan index fit the key's t range [-16,15])
 *   out_dev   : float32 [n, out_channels] with row stride `ldo` floats (>= out_channels)
 *   activation: 0 = raw logits, 1 = sigmoid */
int sps_head_num_tensors(int out_channels);
int sps_head_tensor_info(int out_channels, int idx, char *name, int name_cap, int64_t *offset, int64_t *numel);
int64_t sps_head_numel(int out_channels);
int sps_weights_load_head(sps_ctx *ctx, const float *blob_host, int64_t numel, int out_channels);
int sps_forward_head(sps_ctx *ctx, const float *coords_dev, int64_t ld, int64_t n, float voxel_size,
                     const float *feats_dev, float t_base, float *out_dev, int64_t ldo, int activation, void *stream);

/* ---- metrics ------------------------------------------------------------------------
 * Replaces the per-scan part of SPSNet.predict_step (reference models.py:84-105) +
 * util.calculate_metrics (util.py:285-299).  For every batch index b < n_batches it
 * accumulates over the rows with t == 1 (scan rows):
 *   out[b*8+0..7] = count, TP, FP, FN, TN, sum (s-g)^2, sum g, sum g^2
 * with pred = s < eps ? 0 : 1, gt = g < eps ? 0 : 1 (float32 compares), positive = 1.
 *   batch_dev : float32 rows (b,x,y,z,t,label) with row stride ld (ld >= 6)
 * Synchronises `stream` (copies 8*n_batches doubles to out_host). */
int sps_metrics(sps_ctx *ctx, const float *scores_dev, const float *batch_dev, int64_t ld, int64_t n,
                float eps, int n_batches, double *out_host, void *stream);

/* Same accumulators written to DEVICE memory out_dev[n_batches*8] (doubles) without synchronising:
 * lets a streaming loop keep per-scan metric rows on the device and gather them once per sequence
 * (RCCL all-gather in the multi-GPU predict loop). */
int sps_metrics_dev(sps_ctx *ctx, const float *scores_dev, const float *batch_dev, int64_t ld, int64_t n,
                    float eps, int n_batches, double *out_dev, void *stream);

/* ---- variant-B submap (online path) ---------------------------------------------------
 * Replaces util.to_coords_features + util.prune (reference util.py:67-114): voxel =
 * trunc(xyz / ds) in f32; the map's unique voxel set is kept in a device-resident hash
 * (the reference rebuilds it every callback, util.py:86-89). */
int sps_map_upload(sps_ctx *ctx, const float *map_xyz_dev, int64_t ld, int64_t m, float ds, void *stream);
/* Same, from int32 voxel indices [m,3] already produced by util.to_coords_features
 * (reference util.py:75: (xyz/ds).int()), row stride ld ints. */
int sps_map_upload_voxels(sps_ctx *ctx, const int32_t *map_ijk_dev, int64_t ld, int64_t m, void *stream);
/* out_xyz_dev must hold n rows of 3 floats.  Writes the voxel corners (ix*ds, f32) of
 * (unique scan voxels INTERSECT map voxels) in scan first-occurrence order.
 * Synchronises; *n_sub = rows written, *n_scan_vox = number of unique scan voxels.
 * The float form truncates xyz/ds itself with the ds given to sps_map_upload. */
int sps_submap_voxel(sps_ctx *ctx, const float *scan_xyz_dev, int64_t ld, int64_t n, float *out_xyz_dev,
                     int64_t *n_sub, int64_t *n_scan_vox, void *stream);
int sps_submap_voxel_ijk(sps_ctx *ctx, const int32_t *scan_ijk_dev, int64_t ld, int64_t n, float ds,
                         float *out_xyz_dev, int64_t *n_sub, int64_t *n_scan_vox, void *stream);

/* ---- streaming filter (online path, stream-ordered end to end) --------------------------------
 * The per-scan body of the reference's ROS node (c_ws/src/sps_filter/scripts/sps_node.py:88-176) without the
 * transport, as four stream-ordered calls that never synchronise with the host: the row counts they produce stay in
 * a caller-owned device array counts_dev (int32[4]) that the caller reads back ONCE, after the whole scan was issued.
 *
 * sps_transform_points: util.transform_point_cloud (reference util.py:187-194; sps_node.py:103, blt_dataset.py:69-70):
 *   p' = T [p;1] with perspective divide in float64 (fused multiply-add chain over k = 0..3, the order numpy's dgemm
 *   uses: bit-identical to the reference in float64), stored as float32 (out_f64 = 0; sps_node.py:107) or float64.
 *   xyz_dev rows are float32 (in_f64 = 0) or float64 (in_f64 = 1) with row stride ld; T_host is the row-major 4x4
 *   matrix ON THE HOST (passed by value to the kernel: no copy), NULL = identity.
 * sps_filter_prepare: sps_node.py:103-117 + the tensor assembly of util.infer (util.py:163-176).  Writes into
 *   batch_dev (float32 [2n, 5], caller-owned) the rows (0, x', y', z', 1) of the transformed scan followed by the rows
 *   (0, vx, vy, vz, 0) of the variant-B submap (voxel corners of scan voxels INTERSECT map voxels, scan
 *   first-occurrence order, as sps_submap_voxel), and counts_dev[0] = n_sub, [1] = n_scan_vox, [2] = n + n_sub.
 *   Needs sps_map_upload (float form).
 * sps_forward_n: sps_forward whose row count is read from DEVICE memory (*n_dev <= n_max; grids are sized for
 *   n_max); scores_dev [n_max], rows >= *n_dev are left untouched.
 * sps_compact_stable: the epsilon filter `scan[scores <= eps]` (sps_node.py:147-148): copies, in input order, the
 *   first `cols` floats of every row i < n of rows_dev (row stride ld) whose score is <= eps to out_dev [., cols];
 *   *count_dev = rows kept (NaN scores are dropped). */
int sps_transform_points(sps_ctx *ctx, const void *xyz_dev, int in_f64, int64_t ld, int64_t n, const double *T_host,
                         void *out_dev, int out_f64, int64_t ldo, void *stream);
int sps_filter_prepare(sps_ctx *ctx, const void *raw_xyz_dev, int in_f64, int64_t ld, int64_t n, const double *T_host,
                       float *batch_dev, int32_t *counts_dev, void *stream);
int sps_forward_n(sps_ctx *ctx, const float *coords_dev, int64_t ld, int64_t n_max, const int32_t *n_dev, float voxel_size,
                  float *scores_dev, void *stream);
int sps_compact_stable(sps_ctx *ctx, const float *scores_dev, const float *rows_dev, int64_t ld, int cols, int64_t n,
                       float eps, float *out_dev, int32_t *count_dev, void *stream);
/* sps_filter_finish: everything else the reference's two SPS nodes publish and log from the scores of a frame
 * (sps_node.py:123-161, sps_node_cvm.py:145-184), in TWO launches, stream-ordered, no host synchronisation, no atomics
 * (positions and sums are combined from per-workgroup partials in a fixed order: two calls on the same input give the
 * same bits).  Takes the place of sps_compact_stable in a frame that wants the node's full output.
 *   scores_dev [n]; raw_dev: the scan rows AS RECEIVED, float32, row stride ld, cols floats per row; label_col: the
 *   column of raw_dev that holds the label (sps_node.py:107: 3), or -1 for a scan without labels; batch_dev / counts_dev:
 *   what sps_filter_prepare wrote for this scan (n rows (0, x', y', z', 1), then counts_dev[0] rows (0, vx, vy, vz, 0)).
 *   keep_strict = 0 keeps score <= eps (sps_node.py:148); keep_strict = 1 keeps score < eps, the rows with pred == 0
 *   (sps_node_cvm.py:171): a score exactly eps is kept by the first node and dropped by the second.  Float32 compares.
 * Outputs, each may be NULL (filtered_dev and count_dev go together):
 *   filtered_dev [., cols]  the whole kept rows in input order, *count_dev = their number (a NaN score is dropped);
 *   labels_dev   [n] int32  pred = score < eps ? 0 : 1 (a NaN score gives 1, as np.where does);
 *   cloud_tr_dev [n, 4]     (x', y', z', (float)pred)   -- debug/raw_cloud_tr;
 *   submap_dev   [n_sub, 4] (vx, vy, vz, 1), n_sub = counts_dev[0] read on the device -- debug/cloud_submap;
 *   sums_dev     [8] f64    the accumulator row of sps_metrics_dev over all n rows with gt = label < eps ? 0 : 1;
 *                           written only when label_col >= 0.
 * n = 0 writes *count_dev = 0 and a zero sums row. */
int sps_filter_finish(sps_ctx *ctx, const float *scores_dev, int64_t n, const float *raw_dev, int64_t ld, int cols,
                      int label_col, const float *batch_dev, const int32_t *counts_dev, float eps, int keep_strict,
                      float *filtered_dev, int32_t *count_dev, int32_t *labels_dev, float *cloud_tr_dev, float *submap_dev,
                      double *sums_dev, void *stream);

/* ---- variant-A submap (offline path) ----------------------------------------------------
 * Replaces BacchusDataset.select_closest_points (reference src/sps/datasets/blt_dataset.py:258-271:
 * scipy cKDTree.query_ball_tree(map_tree, r = VOXEL_SIZE)): for every scan point the indices of the
 * map points within Euclidean distance r (closed ball, float64), one hit list per scan point,
 * concatenated in scan-point order with duplicates kept; inside a list the hits are ordered by
 * neighbour cell ((dx+1) + 3(dy+1) + 9(dz+1)), ascending map index inside a cell (scipy's in-list
 * order is the tree's traversal order, i.e. unspecified).
 * The map is binned by the caller into cells of size cell_size >= r: cell_keys (u64, see
 * sps_amd/datasets/blt_dataset.py), cell_start [n_cells+1], cell_pts [m] (map indices grouped by cell),
 * map_xyz float64 [m,3] compact.  The ctx keeps device copies.  Synchronises.
 * Cell index: floor(v / cell_size) per axis, a float64 division -- the keys must be built with that rule, and every
 * query (sps_radius_count / _fill / _item, sps_loc_align) finds the cell of its point with it, as the uploaded keys.
 * (A product with 1 / cell_size is NOT the same rule: it differs by one cell next to a face.) */
int sps_radius_grid_upload(sps_ctx *ctx, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                           const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t m,
                           double cell_size, double r, void *stream);
/* counts_dev[i*27 + c] = number of hits of scan point i in its neighbour cell c (float64 rows xyz...,
 * row stride ld); counts_dev holds 27*n ints. */
int sps_radius_count(sps_ctx *ctx, const double *scan_xyz_dev, int64_t ld, int64_t n, int32_t *counts_dev, void *stream);
/* Writes the hits of (point i, cell c) at out_idx_dev[offsets_dev[i*27 + c] ...] (offsets = exclusive prefix
 * sum of the 27*n counts, computed by the caller), so a point's list is contiguous. */
int sps_radius_fill(sps_ctx *ctx, const double *scan_xyz_dev, int64_t ld, int64_t n, const int64_t *offsets_dev,
                    int64_t *out_idx_dev, void *stream);

/* A second context of the same device uses the owner's radius grid without a copy (a view: the owner keeps and frees
 * the allocations and must outlive it).  The S pipelined contexts of one evaluation loop share ONE grid this way. */
int sps_radius_grid_attach(sps_ctx *ctx, sps_ctx *owner);
/* The whole offline item on the device, stream-ordered, no host synchronisation: replaces BacchusDataset.__getitem__
 * (reference src/sps/datasets/blt_dataset.py:209-244: scan rows + add_timestamp + select_closest_points + map rows) and
 * the batch column of BacchusModule.collate_fn (:173-182).  scan_dev rows are (x, y, z, label) in the scan's own dtype
 * (float64: in_f64 = 1, else float32, promoted to float64 for the radius test as cKDTree does), row stride ld >= 4.
 * Writes into rows_dev (float32 [row_cap, ldo], ldo >= 6), starting at row *row_off_dev (NULL = 0):
 *   n rows (b, x, y, z, 1, label)   then   m rows (b, mx, my, mz, 0, 1)
 * with b = batch_index and the m map points within r of some scan point (one list per scan point, duplicates kept, as
 * sps_radius_count / sps_radius_fill), and *n_rows_dev = *row_off_dev + n + m: chaining calls with
 * row_off_dev = n_rows_dev appends the items of a batch.  Rows beyond row_cap are dropped and the next synchronising
 * call (sps_check) returns SPS_ERR_ITEMCAP. */
int sps_radius_item(sps_ctx *ctx, const void *scan_dev, int in_f64, int64_t ld, int64_t n, float batch_index,
                    const int32_t *row_off_dev, float *rows_dev, int64_t ldo, int64_t row_cap, int32_t *n_rows_dev,
                    void *stream);
/* sps_forward_metrics whose row count is read from DEVICE memory (*n_dev <= n_max; grids are sized for n_max): the
 * consumer of sps_radius_item in the offline loop (reference scripts/predict.py:64-67 -> models.py:84-111). */
int sps_forward_metrics_n(sps_ctx *ctx, const float *batch_dev, int64_t ld, int64_t n_max, const int32_t *n_dev,
                          float voxel_size, float eps, int n_batches, float *scores_dev, double *out_dev, void *stream);

/* ---- training step ---------------------------------------------------------
 * Replaces the forward + loss.backward() of SPSNet.training_step / common_step (reference
 * src/sps/models/models.py:62-82) for the network part; the loss (nn.MSELoss on the scan rows) and the optimiser
 * (Adam + StepLR, models.py:154-160) stay with the caller.
 * sps_train_forward: params_dev is the flat parameter blob ON THE DEVICE in the layout of sps_weights_tensor_info
 *   (kernels [K][C_in][C_out], BN weight / bias / running_mean / running_var, final.bias); the running statistics are
 *   ignored: BatchNorm normalises with the batch statistics of the active rows (train mode, eps = 1e-5) and
 *   batch_stats_dev (optional, [3 * sum of BN widths] floats: per conv in layer order the batch mean, the BIASED
 *   and the UNBIASED batch variance of its BN) lets the caller update running_mean / running_var as nn.BatchNorm1d does.  scores_dev [n]
 *   = sigmoid(final(...)) sliced to the points, as sps_forward.  The activations the backward needs stay in ctx.
 * sps_train_backward: dscores_dev [n] = d(loss)/d(scores); scores_dev the forward's output; grad_dev receives
 *   d(loss)/d(parameter) in the blob layout (zeros in the running-statistics slots).  Deterministic (fixed-order
 *   reductions).  Stream-ordered, no host synchronisation. */
int sps_train_forward(sps_ctx *ctx, const float *params_dev, int64_t numel, const float *coords_dev, int64_t ld, int64_t n,
                      float voxel_size, float *scores_dev, float *batch_stats_dev, void *stream);
int sps_train_backward(sps_ctx *ctx, const float *dscores_dev, const float *scores_dev, float *grad_dev, int64_t numel,
                       void *stream);
/* The activations, kernel maps and parameter copy a backward reads live in ctx and belong to ONE forward: every forward
 * of the context (training or inference) bumps its generation.  sps_train_generation returns the generation of the
 * training forward whose activations are held (what torch keeps in the autograd node, sps_amd/models/models.py
 * ::_TrainForward); sps_train_backward_at is sps_train_backward that fails with SPS_ERR_INVALID when that forward's
 * activations have been overwritten by a later forward (two graphs alive on one context, an evaluation forward
 * issued mid-step) instead of returning gradients of the wrong forward.  sps_train_backward itself refuses a backward
 * after an intervening inference forward.
 * Train-mode BatchNorm needs more than one active row per level (nn.BatchNorm1d raises "Expected more than 1 value per
 * channel when training", reference resnet.py:100-107): a training forward whose coarsest level has a single voxel sets a
 * sticky flag and the next synchronising call (sps_check) returns SPS_ERR_INVALID.
 * The loss gradient: the backward adds dscores[p] * s_p * (1 - s_p) per voxel in 32.32 fixed point (sums independent of the
 * arrival order), so every term of a row that has a voxel must be finite with |term| <= 32768 (out-of-range rows, whose
 * score is NaN, contribute nothing and their dscores are not read); terms below 2^-33 round to zero.  A NaN, an infinity
 * or a larger term (a diverged loss) sets a sticky flag of its own: the next synchronising call returns SPS_ERR_INVALID with
 * a message that names the loss gradient, and the gradients of that step are unspecified (autograd would return NaN). */
int sps_train_generation(sps_ctx *ctx, int64_t *generation);
/* Introspection (tests): the launch plan of the weight gradient of convolution `conv_name` (state_dict name without
 * ".kernel"; not conv0p1s1 or final) at the context's current capacity, valid after a training forward: *gshift = 4 or 6
 * (rows read 16 or 64 at a time), *nwg = workgroups per (offset, channel block) (> 1: partial sums reduced at the end). */
int sps_train_wgrad_plan(sps_ctx *ctx, const char *conv_name, int32_t *gshift, int32_t *nwg);
int sps_train_backward_at(sps_ctx *ctx, int64_t generation, const float *dscores_dev, const float *scores_dev,
                          float *grad_dev, int64_t numel, void *stream);

/* The loss of common_step (reference src/sps/models/models.py:62-72): nn.MSELoss between the scores and the labels of the
 * rows whose time index is 1 (the scan; the reference selects them with np.where on the host), and the R2Score the same
 * step logs.  sps_scan_mse: scores_dev [n]; labels_dev / t_dev point at the label / time column of the batch rows (row
 * strides ld_labels / ld_t in floats); work_dev [4 * 257] doubles (scratch the backward reads: work[0] = the number of
 * selected rows); out_dev [2] floats = loss, R2.  sps_scan_mse_backward: dscores_dev [n] = gloss * d loss / d scores
 * (gloss_dev: one float on the device).  f64 sums in a fixed order; stream-ordered, no host synchronisation; no context
 * (the caller has made the device current). */
int sps_scan_mse(const float *scores_dev, const float *labels_dev, int64_t ld_labels, const float *t_dev, int64_t ld_t, int64_t n,
                 double *work_dev, float *out_dev, void *stream);
int sps_scan_mse_backward(const float *scores_dev, const float *labels_dev, int64_t ld_labels, const float *t_dev, int64_t ld_t,
                          int64_t n, const double *work_dev, const float *gloss_dev, float *dscores_dev, void *stream);

/* ---- per-stage timing (hipEvents on the caller's stream; for bench.py / DESIGN.md) ------
 * With profiling on, sps_forward records one event after every stage ("reset", "voxelize",
 * "pyramid", "maps", one per convolution by state_dict name, "slice_sigmoid").  After a forward,
 * sps_profile_count gives the number of stages and sps_profile_read(i) synchronises on stage i's
 * closing event and returns its name and duration in milliseconds.  Replaces the reference's
 * time.time() deltas (util.py:164,182; sps_node.py:164-176). */
int sps_profile_enable(sps_ctx *ctx, int on);
int sps_profile_count(sps_ctx *ctx);
int sps_profile_read(sps_ctx *ctx, int idx, char *name, int name_cap, float *ms);
/* The kernel (class) stage idx launched, e.g. "k_conv_px", "k_conv<3x3x3x3, levels 2-4>", "k_upconv", "k_maps": lets
 * bench.py aggregate the stages per kernel the way `rocprofv3 --stats` does. */
int sps_profile_kernel(sps_ctx *ctx, int idx, char *name, int name_cap);

/* ---- introspection (parity tests; all synchronise) ----------------------------------- */
/* Number of active voxels at each tensor stride of the last forward. */
int sps_level_counts(sps_ctx *ctx, int64_t counts_host[SPS_NUM_LEVELS]);
/* Integer coordinates [V,5] (b,x,y,z,t) of level `level` (0 = tensor stride 1). */
int sps_get_voxels(sps_ctx *ctx, int level, int32_t *coords_dev);
/* Debug view of the block hash of level `level` after the last forward: the number of slots of the level's table, the
 * number of 4x4x4 blocks, and (bslot_host non-null, room for `cap` entries) the slot each block held, by block rank
 * (first-occurrence order; the voxel rows of sps_get_voxels are block-contiguous in that order).  Read-only. */
int sps_get_block_slots(sps_ctx *ctx, int level, int64_t *n_slots, int64_t *n_blocks, int32_t *bslot_host, int64_t cap);
/* inverse map point -> ts1 voxel row, int64 [n] (-1 for out-of-range rows). */
int sps_get_inverse(sps_ctx *ctx, int64_t *inv_dev);
/* parent row (level+1) of each voxel of `level` (0..3), int32 [V_level]. */
int sps_get_parent(sps_ctx *ctx, int level, int32_t *parent_dev);
/* Kernel-map pair counts: which = 0..4 -> 3x3x3x3 map at level which; 5 -> 5x5x5x1 map at
 * level 0.  pairs_host[k] = number of (in,out) pairs of offset k (81 or 125 entries). */
int sps_get_map_pairs(sps_ctx *ctx, int which, int64_t *pairs_host);
/* Present-offset masks of the 16-row output tiles of a kernel map (which as above): uint32
 * [n_tiles][4].  which = 0..4 (3x3x3x3): one word per time slice, offset k = 27 * word + bit (word 3 unused);
 * which = 5: bit k of the 128-bit field.  A set bit = some row of the tile has a neighbour through offset k. */
int sps_get_tile_masks(sps_ctx *ctx, int which, uint32_t *masks_dev, int64_t *n_tiles);
/* The 3x3x3x3 neighbour table of level `which` (0..4), int32 [81][V] compact; entries of (tile, k)
 * pairs whose tile-mask bit is clear are unspecified (never written, never read by the convolution). */
int sps_get_nbr(sps_ctx *ctx, int which, int32_t *nbr_dev);
/* A kernel map of the last forward as ME holds it (the set of (input row, output row) pairs per kernel offset; reached from
 * /root/reference/src/sps/models/MinkowskiEngine/minkunet.py:162-217), exported as a dense int32 table [K][V_out] compact:
 * out[k * V_out + u] = input row paired with output row u through offset k, or -1.
 *   which = 0..4: 3x3x3x3 map of level which (K = 81, k = (dx+1) + 3(dy+1) + 9(dz+1) + 27(dt+1));
 *   which = 5:    5x5x5x1 map of level 0 (K = 125; materialised for this call -- conv0 derives the same presence bits from the
 *                 block tables without ever storing the map);
 *   which = 6..9: stride-2 map into coarse level which - 5 (K = 8, k = dx + 2dy + 4dz; rows = coarse voxels, entries = fine
 *                 rows; the transposed convolutions read the same table with the roles swapped).
 * source = 0: the output-stationary neighbour / child table; source = 1 (which = 0..4 at the pair-exact levels): decoded from
 * the RULEBOOK the pair-exact convolutions read; *n_entries (may be NULL) = number of pairs it holds (malformed or duplicate
 * entries fail the call). */
int sps_get_kernel_map(sps_ctx *ctx, int which, int source, int32_t *out_dev, int64_t *n_entries);
/* Chunks of the rulebook of level `which` (a pair-exact level) per 64-row supertile and time slice, int32
 * [n_supertiles][3] on the host: what the pair-exact convolutions execute (one chunk = 16 pair slots).  chunks_host may be
 * NULL (only *n_supertiles is set). */
int sps_get_rulebook_chunks(sps_ctx *ctx, int which, int32_t *chunks_host, int64_t *n_supertiles);
/* What the last forward launched for the layer `conv_name` of the wiring table (a state_dict name without ".kernel":
 * "conv0p1s1", "block3.0.conv1", "convtr6p4s2", ...): the record of the decisions taken at launch time, not a second
 * evaluation of the geometry rule.  Host only, no synchronisation.
 *   out[0] kernel family (SPS_LAUNCH_*; SPS_LAUNCH_NONE: the layer had no launch of its own -- a transposed convolution that
 *          ran in the epilogue of the layer before it, or a forward that stopped earlier)
 *   out[1] column tiles per wave (ntw)          out[2] splits of a tile's unit list (S)
 *   out[3] 1 = the scalar-counter unit loop (U4) out[4] 1 = the next layer's transposed convolution ran in this launch
 *   out[5] positions per tier of the balanced tile order (order_ways; 0 = tiles in row order)
 *   out[6] arena capacity in rows the geometry was decided from
 *   out[7] 1 = the context was marked pipelined (sps_ctx_set_pipelined) */
#define SPS_LAUNCH_NONE 0
#define SPS_LAUNCH_CONV 1    /* k_conv */
#define SPS_LAUNCH_CONV_PX 2 /* k_conv_px */
#define SPS_LAUNCH_UPCONV 3  /* k_upconv */
#define SPS_LAUNCH_CONV0 4   /* k_conv0_fused / k_conv0_feat */
int sps_get_conv_launch(sps_ctx *ctx, const char *conv_name, int32_t out[8]);
/* Per-voxel logits of the last forward, float32 [V_0]. */
int sps_get_logits(sps_ctx *ctx, float *logits_dev);
/* Named intermediate feature maps: "out_p1","block1".."block8"; copies [V,C] row-major
 * f32 (compact, ld = C) into out_dev; *rows,*cols describe it. */
int sps_get_feature(sps_ctx *ctx, const char *name, float *out_dev, int64_t *rows, int64_t *cols);


/* ---- LTS baseline (SPCTReg offset-attention regressor) ------------------------------------------------------------
 * The reference's third learned baseline, c_ws/src/inference_model/lts_filter/scripts/:
 *   sps_lts_project : Loader.lidar_to_image + __getitem__ (loader.py:36-59, :62-72): range-image projection of a cloud
 *                     and its split into windows of N = beams x window_size cells;
 *   sps_lts_forward : SPCTReg.forward (transformer.py:97-138) in f32, BatchNorm in eval mode (folded at create),
 *                     dropout = identity; the N x N attention of each OA block (transformer.py:51-67) is never stored;
 *   the node's metrics and epsilon filter (stability_filter.py:160-193) reuse sps_metrics_dev / sps_compact_stable on
 *   the metric rows sps_lts_project writes.
 * Weight blob: the reference state_dict, every key in its order (sps_lts_tensor_info), num_batches_tracked as one float.
 * q_conv.weight and k_conv.weight are one Parameter in the reference: the k_conv entry is used (it is loaded second).
 * No function here synchronises except sps_lts_check.  A handle is not thread-safe; its workspace is reused by every
 * forward (one forward in flight per handle). */
typedef struct sps_lts sps_lts;
#define SPS_LTS_VLP16 0 /* 16 beams, fov +-16.8 deg, window 128 -> 8 windows of N = 2048 */
#define SPS_LTS_HDL32 1 /* 32 beams, fov +30 / -10 deg, window 64 -> 16 windows of N = 2048 */
int sps_lts_num_tensors(void);
/* name, offset / numel in floats, shape[3] (unused dims 0), ndim (0 for a scalar) of blob tensor idx; any out may be NULL */
int sps_lts_tensor_info(int idx, char *name, int name_cap, int64_t *offset, int64_t *numel, int64_t *shape, int *ndim);
int64_t sps_lts_numel(void);
int sps_lts_lidar_info(int lidar, int *beams, int *window, int *num_windows);
/* blob_host: sps_lts_numel() floats on the host, or NULL for a projection-only handle.  Synchronises (uploads the
 * folded weights). */
int sps_lts_create(int device, const float *blob_host, int64_t numel, sps_lts **out);
int sps_lts_destroy(sps_lts *h);
/* pts_dev: n rows (x, y, z, s, ...) f32 with row stride ld >= 4; rows with s == -1 are dropped; per cell the
 * lexicographically largest (x, y, z, s) row is kept (np.unique + last write wins; -0.0 == +0.0).
 * frame_dev [beams][1024][4] (required); x_dev [num_windows][3][N] (the network input, may be NULL);
 * rows_dev [num_windows * N][6] = (0, x, y, z, 1, s) per cell, empty cells (0, 0, 0, 0, 1, 0) (sps_metrics_dev /
 * sps_compact_stable input, may be NULL).  A row whose elevation index is outside [-beams, beams) or with a NaN coordinate
 * (IndexError in the reference) sets the handle's sticky status, reported by sps_lts_check. */
int sps_lts_project(sps_lts *h, const float *pts_dev, int64_t ld, int64_t n, int lidar, float *frame_dev, float *x_dev,
                    float *rows_dev, void *stream);
/* x_dev [B][3][N] f32 (torch layout of the reference's input), scores_dev [B][N] = sigmoid output; any B >= 1, N >= 1. */
int sps_lts_forward(sps_lts *h, const float *x_dev, int64_t B, int64_t N, float *scores_dev, void *stream);
/* Synchronises `stream`; SPS_ERR_RANGE if a projection since the last check met an out-of-image or NaN point (then clears). */
int sps_lts_check(sps_lts *h, void *stream);
/* Intermediate of the last forward: which = 0 embedding, 1..4 outputs of sa1..sa4 (f32 [B*N][128], point-major),
 * 5 / 6 linear1's max / mean over the points of each window (f32 [B][2048]).  out_dev NULL: *rows, *cols only. */
int sps_lts_tap(sps_lts *h, int which, float *out_dev, int64_t *rows, int64_t *cols, void *stream);

/* ---- online baseline filters (4DMOS, MapMOS, mask) ------------------------------------------------------------------
 * The per-frame bodies of the reference's other scan filters (c_ws/src/mos4d/scripts/mos4d_node.py:80-147,
 * c_ws/src/mapmos/scripts/mapmos_node.py:70-112, c_ws/src/sps_filter/scripts/mask.py:86-147) as stream-ordered calls that
 * never synchronise with the host; the row counts they produce stay in caller-owned device int32 arrays.
 *
 * sps_forward_head_n: sps_forward_head whose row count is read from DEVICE memory (*n_dev <= n_max; grids are sized for
 *   n_max): MapMOSNet.predict (mapmos.py:59-83, mapmos_node.py:95) on scan rows + a radius crop whose size only the device
 *   knows.  Rows at or past *n_dev of out_dev are left untouched; *n_dev == 0 is a valid (empty) forward.
 * sps_transform_rows: the window / batch rows of the baselines -- util.transform_point_cloud (util.py:187-194, the f64
 *   fused multiply-add chain of sps_transform_points) stored as float32 rows (0, x', y', z', t) with row stride ldo >= 5:
 *   t = the scan index (mos4d_node.py:97-104, then .to(float32) at :113) or 0 (the MapMOS scan, mapmos.py:39-47).
 *   feat_dev (may be NULL): feat_dev[i] = feat_value (the MapMOS per-point feature, mapmos.py:64-71).
 * sps_transform_points_n: sps_transform_points whose row count is read from device memory (*n_dev <= n_max): the mask
 *   node's inverse transform of the submap that sps_filter_prepare left behind the scan rows (mask.py:121-125,
 *   util.inverse_transform_point_cloud: pass T_host = inv(T) computed on the host as np.linalg.inv does).
 * sps_radius_crop: select_points_within_radius (mapmos_node.py:63-68, :79-80, r = 30): map point i is kept iff
 *   sqrt((dx*dx + dy*dy) + dz*dz) <= r with d = p_i - T[:3, 3], every operation a rounded float64 one (numpy's order;
 *   float32 maps are widened first).  The kept points, in ascending map index (np.where), become rows n_scan + k of
 *   rows_dev: (0, x, y, z, -1) as float32, and feat_dev[n_scan + k] = feat_value (feat_dev may be NULL).
 *   counts_dev[0] = min(kept, cap), counts_dev[1] = n_scan + counts_dev[0].  More than cap kept points: the rest are
 *   dropped and the next sps_check returns SPS_ERR_ITEMCAP.  scratch_dev: int32[max(1, ceil(m / SPS_CROP_BLOCK))].
 *   map_dev rows are float32 (in_f64 = 0) or float64 with row stride ld >= 3; T_host NULL = centre at the origin.
 * sps_label_filter: to_label + `scan[labels == 0]` (mos4d_node.py:121-127, mapmos_node.py:98-103): labels_dev[i] = 1 if
 *   logits_dev[i * ld_logits] > 0 else 0 (NaN -> 0); the first three floats of every row i of rows_dev (stride ld) with
 *   label 0 go, in input order, to out_dev [., 4] as (x, y, z, 0); counts_dev[0] = rows kept.  gt_dev (may be NULL): the
 *   ground-truth column (stride ld_gt), gt = s < 0.84f ? 0 : 1 (mos4d_node.py:83), counts_dev[1..4] = TP, FP, FN, TN of
 *   util.calculate_metrics (util.py:285-299, positive = 1; integers, deterministic).  counts_dev holds 5 int32. */
#define SPS_CROP_BLOCK 1024
int sps_forward_head_n(sps_ctx *ctx, const float *coords_dev, int64_t ld, int64_t n_max, const int32_t *n_dev,
                       float voxel_size, const float *feats_dev, float t_base, float *out_dev, int64_t ldo, int activation,
                       void *stream);
int sps_transform_rows(sps_ctx *ctx, const void *xyz_dev, int in_f64, int64_t ld, int64_t n, const double *T_host, float t,
                       float *rows_dev, int64_t ldo, float *feat_dev, float feat_value, void *stream);
int sps_transform_points_n(sps_ctx *ctx, const void *xyz_dev, int in_f64, int64_t ld, int64_t n_max, const int32_t *n_dev,
                           const double *T_host, void *out_dev, int out_f64, int64_t ldo, void *stream);
int sps_radius_crop(sps_ctx *ctx, const void *map_dev, int in_f64, int64_t ld, int64_t m, const double *T_host, double r,
                    int32_t *scratch_dev, int64_t n_scan, float *rows_dev, int64_t ldo, int64_t cap, float *feat_dev,
                    float feat_value, int32_t *counts_dev, void *stream);
int sps_label_filter(sps_ctx *ctx, const float *logits_dev, int64_t ld_logits, int64_t n, const float *rows_dev, int64_t ld,
                     const float *gt_dev, int64_t ld_gt, float *labels_dev, float *out_dev, int32_t *counts_dev, void *stream);

/* ---- localiser (scan-to-map point-to-point ICP) ---------------------------------------------------------------------
 * The stage the reference's localisation experiment puts behind a scan filter (exp_pipeline/loc_exp_general.bash runs
 * hdl_localization there, an external package).  This is NOT a port of it -- no NDT, no UKF, no IMU -- but a
 * deterministic point-to-point ICP that plays the same role: the filter's kept rows are registered against the map and
 * the corrected pose goes back into the filter.  Both calls are stream-ordered and never synchronise with the host;
 * their scratch is the caller's.  No float atomics: float sums go through per-workgroup partial rows combined in block
 * order, so two calls on the same input give the same bits.  Degenerate input never raises the context's sticky error.
 *
 * sps_loc_downsample: voxel-grid thinning of rows_dev (f32 rows (x, y, z, ...), row stride ld >= 3), of which the first
 *   min(*n_dev, n_max) are read (n_dev: the kept-row count sps_filter_finish / sps_label_filter left on the device).
 *   A row's voxel is floor(double(v) / leaf) per axis; of the rows of one voxel the one with the lowest index survives.
 *   The survivors go, in ascending row order, to out_xyz_dev as f64 [cap][3]; survivors beyond cap are dropped and
 *   *count_dev = min(survivors, cap).  A row with a coordinate outside the key range (|voxel| >= 2^20, NaN) is skipped.
 *   scratch_dev: sps_loc_downsample_scratch(n_max) bytes.
 * sps_loc_align: `iters` iterations of point-to-point ICP of pts_dev (f64 [cap][3], the first min(*n_dev, cap) used)
 *   against the map of the context's radius grid (sps_radius_grid_upload with cell_size = r = the correspondence
 *   distance), starting from the row-major 4x4 T_init_host.  Two launches per iteration:
 *     A: q = R p + t as ((r0*x + r1*y) + r2*z) + t; the nearest map point m over the 27 cells around q (cell index
 *        floor(v / cell_size) per axis, as the uploaded keys) with
 *        d2 = (ex*ex + ey*ey) + ez*ez <= r*r, e = q - m, ties to the lowest map index; the terms of H = sum J^T J and
 *        g = sum J^T e with J = [ -[q]x | I ] (unknown delta = (omega, v)), each entry as (a0*b0 + a1*b1) + a2*b2 over
 *        the three residual rows; one partial row per workgroup, added in point order.
 *     B: the partial rows added in block order; n_corr < min_corr -> status 2; Cholesky of H (a pivot <= 0 or a
 *        non-finite solution -> status 3); H delta = -g; Exp(omega) by Rodrigues (first order below |omega| < 1e-12);
 *        T <- [Exp(omega), v; 0, 1] T; |v| < tol_t and |omega| < tol_r -> status 0.
 *   Every operation is a float64 one rounded on its own.  Once the status is final the remaining launches return at
 *   once.  Outputs (device): T_out_dev double[16]; status_dev int32[4] = (code, iterations run, correspondences of the
 *   last iteration run, 0) with code 0 converged, 1 iterations exhausted, 2 too few correspondences, 3 singular system
 *   -- on 2 and 3 T_out is T_init bit for bit; trace_dev double[iters][4] = (n_corr, sum d2, |v|, |omega|) per iteration
 *   (rows of iterations not run are 0); normal_dev (may be NULL) double[iters][28] = the 21 upper-triangle entries of H
 *   row-major, the 6 entries of b = -g, sum d2.  scratch_dev: sps_loc_align_scratch(cap) bytes. */
int64_t sps_loc_downsample_scratch(int64_t n_max);
int64_t sps_loc_align_scratch(int64_t cap);
int sps_loc_downsample(sps_ctx *ctx, const float *rows_dev, int64_t ld, int64_t n_max, const int32_t *n_dev, double leaf,
                       double *out_xyz_dev, int64_t cap, int32_t *count_dev, void *scratch_dev, void *stream);
int sps_loc_align(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host,
                  int iters, int min_corr, double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev,
                  double *trace_dev, double *normal_dev, void *scratch_dev, void *stream);

/* ---- NDT localiser (scan-to-map point-to-distribution registration) --------------------------------------------------
 * The registration hdl_localization runs in the reference's experiment is NDT (ndt_omp: 1 m cells, DIRECT7).  These
 * calls give the localiser above a second association: every map cell carries a mean and an inverse covariance, and a
 * scan point is pulled towards the Gaussians of its own cell and of its six face neighbours.  Thinning
 * (sps_loc_downsample), launch B, the outputs and the status codes are those of sps_loc_align.  Still no UKF, no IMU.
 *
 * sps_ndt_map_build: the map's points grouped by cell of edge `resolution` (cell index floor(v / resolution) per axis;
 *   key, start and cell-ordered point indices as for sps_radius_grid_upload; all device pointers, f64 [n_map][3] points).
 *   Hashes the keys into storage owned by the context and computes per cell, in float64 with sums in the order of the
 *   cell's list: n; the mean; the sample covariance sum (p - mean)(p - mean)^T / (n - 1); its eigen-decomposition by 8
 *   cyclic Jacobi sweeps ((0,1), (0,2), (1,2)); eigenvalues below eig_ratio * lambda_max raised to that value; the
 *   inverse V diag(1 / lambda) V^T as 6 entries (xx, xy, xz, yy, yz, zz).  A cell is valid iff n >= min_points, n >= 2,
 *   lambda_max > 0 and everything is finite; invalid cells stay in the table, flagged, and contribute nothing.  Allocates
 *   and synchronises (like sps_radius_grid_upload); n_map = 0 builds an empty map (every alignment ends with status 2).
 * sps_ndt_map_cells: debug getter -- per cell, in the order of the uploaded keys, the key, n, the mean [3], the inverse
 *   covariance [6] and the valid flag into device arrays (any may be NULL).  Synchronises.
 * sps_ndt_align: as sps_loc_align, with launch A replaced.  Host constants (PCL's), float64: c1 = 10 (1 - outlier_ratio),
 *   c2 = outlier_ratio / resolution^3, d3 = -log c2, d1 = -log(c1 + c2) - d3,
 *   d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1).
 *     A: q = R p + t as in sps_loc_align; cell of q = floor(q / resolution); lookups in the order own cell, +x, -x, +y,
 *        -y, +z, -z (neighbours = 7) or the own cell alone (neighbours = 1).  For a valid cell: x = q - mean,
 *        y = icov x (rows as (m0*x0 + m1*x1) + m2*x2), s = (x0*y0 + x1*y1) + x2*y2, e = exp(-0.5 * (d2 * s)), w = d2 * e;
 *        the cell is skipped unless 0 <= w <= 1 (NaN skips).  With a = (-d1) * w and J = [ -[q]x | I ]:
 *        H(r, c) += a * (J_r . (icov J_c)), g(r) += a * (J_r . y), score += (-d1) * e, every dot product as above; a
 *        point with at least one contributing cell counts once.  Cells are added in lookup order within a point, points
 *        in index order within a workgroup of 32, workgroups as launch B adds them.
 *   H is the positive-semidefinite part of the NDT Hessian and the step H delta = -g is taken at unit length.
 *   trace_dev holds (points counted, score, |v|, |omega|) per iteration, normal_dev the 21 + 6 + 1 sums (b = -g, score).
 *   Status 2: fewer than min_corr points counted.  scratch_dev: sps_ndt_align_scratch(cap) bytes.  Never allocates,
 *   never synchronises, never raises the sticky error. */
int64_t sps_ndt_align_scratch(int64_t cap);
int sps_ndt_map_build(sps_ctx *ctx, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                      const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map,
                      double resolution, int min_points, double eig_ratio, void *stream);
int sps_ndt_map_cells(sps_ctx *ctx, uint64_t *key_out_dev, int32_t *count_out_dev, double *mean_out_dev,
                      double *icov_out_dev, int32_t *valid_out_dev);
int sps_ndt_align(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host,
                  int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                  double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, void *scratch_dev,
                  void *stream);

/* ---- NDT localiser, several hypotheses ------------------------------------------------------------------------------
 * sps_ndt_align from n_hyp start poses in the same launches, and the choice among the end poses by the NDT score.  An
 * alignment that starts in the wrong basin converges there with status 0; the score at the end poses tells the basins
 * apart.  In the reference the registration sits in the hdl() step of exp_pipeline/loc_exp_general.bash
 * (hdl_localization, which ships with a global re-localisation companion for the same need).
 *
 * sps_ndt_align_batch: hypothesis k starts from the row-major 4x4 T_init_dev[k] (a device array: 64 poses do not fit in
 *   a kernel-argument block; the caller leaves it unchanged until the stream has passed the call) and is, operation for
 *   operation and sum for sum, sps_ndt_align from that pose: T_out_dev[k], status_dev[k], trace_dev[k] and normal_dev[k]
 *   have the bits of the single call, T_out_dev[k] is T_init_dev[k] bit for bit on status 2 and 3, and a hypothesis whose
 *   status is final sits out the remaining iterations while the others go on.  The scan points and the map are shared.
 *   Launches: 1 (initialise) + 2 * iters (A with grid (ceil(cap / 32), n_hyp), B with grid n_hyp) + 2:
 *     A once more, for every hypothesis at its final pose whatever its status: final_dev[k] = (score, points counted),
 *        the partial rows added in launch B's block order;
 *     select: the hypothesis with the highest final score among those with status 0 or 1 and at least min_corr points
 *        counted at the final pose; equal scores go to the lowest k.  best_dev = (k, status of k, points counted at its
 *        final pose, n_hyp) and T_best_dev = T_out_dev[k]; where no hypothesis qualifies best_dev = (-1, -1, 0, n_hyp)
 *        and T_best_dev = T_init_dev[0].
 *   Arguments are checked as for sps_ndt_align, and 1 <= n_hyp <= SPS_NDT_MAX_HYP.  trace_dev double[n_hyp][iters][4],
 *   normal_dev (may be NULL) double[n_hyp][iters][28].  scratch_dev: sps_ndt_align_batch_scratch(cap, n_hyp) bytes
 *   (-1 for arguments out of range).  Never allocates, never synchronises, never raises the sticky error. */
#define SPS_NDT_MAX_HYP 64
int64_t sps_ndt_align_batch_scratch(int64_t cap, int n_hyp);
int sps_ndt_align_batch(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_dev,
                        int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                        double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, double *final_dev,
                        int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream);

/* ---- NDT localiser, pose search --------------------------------------------------------------------------------------
 * For a pose known to a few metres and a few tens of degrees (the first frame, the frame after a flagged one, a
 * kidnapped sensor): score a grid of poses, keep the best K <= SPS_NDT_MAX_HYP and hand them to sps_ndt_align_batch,
 * all on the device.  In the reference this is the job of hdl_localization's global re-localisation companion.
 *
 * sps_ndt_score_poses: score_dev[p] = (score, points counted) of the row-major 4x4 pose T_dev[p] for the points
 *   pts_dev[min(*n_dev, cap)][3].  Per point and pose this is step A of sps_ndt_align restricted to its last two sums
 *   (score += (-d1) * e; a point with at least one contributing cell counts once), with its operations, its guards and
 *   its orders: cells in lookup order within a point, points in index order within a workgroup of 32, workgroups as
 *   launch B adds them.  score_dev[p] therefore has the bits of final_dev[k] of sps_ndt_align_batch(iters = 0) started
 *   at T_dev[p].  A pose with a NaN entry, or one that puts every point off the map, scores (0, 0).  An empty map and
 *   *n_dev = 0 are legal: every pose scores (0, 0).  1 <= n_pose <= SPS_NDT_MAX_POSES; neighbours, outlier_ratio and cap
 *   are checked as for sps_ndt_align.  Launches: 2 per chunk of poses.  scratch_dev: sps_ndt_score_scratch(cap, n_pose)
 *   bytes (-1 for arguments out of range) = 16 * ceil(cap / 32) bytes per pose of a chunk; the poses are walked in
 *   chunks so that this stays at or below 64 MiB, or the 32 poses of one tile (512 * ceil(cap / 32) bytes) where those
 *   need more.
 * sps_ndt_top_poses: the k best of n_pose poses by score_dev.  A pose qualifies with count >= min_corr and a score that
 *   is not NaN; the order is (score descending, index ascending), so equal scores keep the lowest index first.
 *   top_index_dev[j] and T_top_dev[j] = T_dev[top_index_dev[j]] for slot j < *n_top_dev = min(k, qualifying poses);
 *   the slots after them get index -1 and the pose of slot 0, and T_dev[0] where nobody qualifies, so that
 *   sps_ndt_align_batch from T_top_dev with n_hyp = k is always well defined.  1 <= k <= SPS_NDT_MAX_HYP.  One launch.
 * Both: never allocate, never synchronise, never raise the sticky error; T_dev stays unchanged until the stream has
 * passed the call. */
#define SPS_NDT_MAX_POSES 65536
int64_t sps_ndt_score_scratch(int64_t cap, int64_t n_pose);
int sps_ndt_score_poses(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_dev,
                        int64_t n_pose, int neighbours, double outlier_ratio, double *score_dev, void *scratch_dev,
                        void *stream);
int sps_ndt_top_poses(sps_ctx *ctx, const double *score_dev, const double *T_dev, int64_t n_pose, int min_corr, int k,
                      int32_t *top_index_dev, double *T_top_dev, int32_t *n_top_dev, void *stream);

/* ---- NDT localiser, online map ----------------------------------------------------------------------------------------
 * A map that grows: the stable points a filter keeps are folded into the cells at the frame's corrected pose, on the
 * frame's stream, so that a localiser can start from an empty map and a scene that changed is learnt.  
 * The context's single map is a pyramid of one level: the calls of this section and of the carving section below are
 * those of the "online pyramid" section with n_levels = 1 on a slot of its own, and share their implementation.
 *
 * sps_ndt_map_build_dynamic: sps_ndt_map_build's arguments and checks, plus cell_capacity >= max(n_cells, 1).  Records,
 *   counts and keys are allocated for cell_capacity cells and the hash for next_pow2(2 * max(512, cell_capacity)) slots (it
 *   never holds more than cell_capacity keys: load <= 0.5).  Per cell the map keeps the moments n (the count), the mean
 *   (the record's) and S = sum (p - mean)(p - mean)^T (6 entries, before the division by n - 1), and a device counter of
 *   the cells assigned.  The first n_cells records have the bits sps_ndt_map_build writes for the same arguments; the
 *   records of unassigned cells are zero (valid = 0) and their keys empty (all bits set), so sps_ndt_align and the batch
 *   and search calls run unchanged.  n_map = 0 builds an empty map to grow from.  Allocates and synchronises.
 *   sps_ndt_map_cells then writes cell_capacity rows.  A map built by sps_ndt_map_build refuses the update (INVALID).
 * sps_ndt_map_update: folds pts_dev[0 .. min(cap, *n_dev)) (f64 [cap][3], sensor frame) into the map at the row-major
 *   4x4 pose T_dev (16 doubles on the device, e.g. T_out_dev of sps_ndt_align) where that is not NULL, else T_host.
 *   gate_dev (may be NULL) points at a device int32: unless it holds 0 or 1 (status_dev[0] of an alignment, best_dev[1]
 *   of a batch) the call changes no byte of the map and info_dev = (cells assigned, 0, 0, 0).  Per point
 *   q = ((r0*x + r1*y) + r2*z) + t; its cell is floor(q / resolution) per axis; a non-finite coordinate or a cell index
 *   beyond +-1048575 skips the point.
 *     New cells: a cell that is not in the map is founded by the lowest point index that falls in it; founders get
 *       consecutive cell ids in ascending founder index from the current count; a founder whose id would reach
 *       cell_capacity founds nothing and the points of its cell are dropped for this update.
 *     Batch: per touched cell n_b, mean_b, S_b over its points in ascending point index, in the operation order of
 *       sps_ndt_map_build (sum, divide, second pass of outer products).
 *     Forgetting (max_cell_points = m; 0 and 1: off): if m >= 2 and the stored n > m, S *= (m - 1) / (n - 1) (one division,
 *       six products) and n = m, before the merge.
 *     Merge: stored n = 0 takes (n_b, mean_b, S_b).  Otherwise n' = n + n_b, delta = mean_b - mean, f = n_b / n',
 *       mean' = mean + delta * f, g = (n * n_b) / n', S'_ij = (S_ij + S_b,ij) + (delta_i * delta_j) * g.  The record is then
 *       written from (n', mean', S') as sps_ndt_map_build writes it (S' / (n' - 1), Jacobi, eigenvalue floor, inverse,
 *       validity with the build's min_points and eig_ratio).  Untouched cells keep every bit.
 *   info_dev int32[4] = (cells assigned after the update, cells founded, cells dropped for capacity in this update,
 *   points integrated).  Seven launches and two memsets of the scratch whatever the data; cap <=
 *   SPS_NDT_UPDATE_MAX_POINTS.  scratch_dev: sps_ndt_map_update_scratch(cap) bytes (-1 for cap out of range), 256-byte
 *   aligned; it is sps_ndt_pyramid_update_scratch(cap, 1).  The result depends on the points, their order and the pose
 *   only.  Never allocates, never synchronises, never raises the sticky error.
 * sps_ndt_map_info: debug -- out_host = (cells assigned, cell_capacity, cells dropped since the build, 0).  Synchronises. */
#define SPS_NDT_UPDATE_MAX_POINTS 65536
int sps_ndt_map_build_dynamic(sps_ctx *ctx, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                              const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map,
                              double resolution, int min_points, double eig_ratio, int64_t cell_capacity, void *stream);
int64_t sps_ndt_map_update_scratch(int64_t cap);
int sps_ndt_map_update(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                       const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev,
                       void *scratch_dev, void *stream);
int sps_ndt_map_info(sps_ctx *ctx, int64_t *out_host);

/* ---- NDT localiser, online map: free-space carving ---------------------------------------------------------------------
 * The other half of a changed scene: what disappeared.  Every point of a frame is the end of a ray from the sensor; a
 * Gaussian that rays pass straight through, frame after frame, while no ray ends in its cell is cleared (the ray-tracing
 * update of NDT occupancy maps, Saarinen et al., reduced to integer counts).    Additive: sps_version() is
 * unchanged.
 *
 * Per-cell state: a map built by sps_ndt_map_build_dynamic also holds three int32[cell_capacity] arrays, zero after the
 *   build: pass and hit, the counts of the last carve whose gate was open, and miss, the consecutive carves in which the
 *   cell was seen through.  sps_ndt_map_build drops them with the rest of the dynamic state.
 * sps_ndt_map_carve: the carve of a pyramid of one level (sps_ndt_pyramid_carve with the scalar end_margin as its one
 *   entry).  pts_dev, n_dev, cap, T_host, T_dev and gate_dev are sps_ndt_map_update's and are checked as there
 *   (cap <= SPS_NDT_UPDATE_MAX_POINTS; a map built by sps_ndt_map_build is refused with INVALID).  end_margin >= 0 and
 *   finite, through_sigma > 0 and finite, min_pass >= 1, miss_frames >= 1, 1 <= max_steps <= 4096, else INVALID.
 *   Gate: unless *gate_dev holds 0 or 1 (NULL: open) no byte of the map and none of the three arrays changes and
 *   info_dev = (0, 0, 0, 0).  With the gate open pass and hit are first set to 0 for every cell.
 *     Ray i < min(cap, *n_dev): origin o = (T[3], T[7], T[11]), end q = ((r0*x + r1*y) + r2*z) + t of point i, direction
 *       d = q - o per axis.  The ray is skipped, and not counted, if a coordinate of q or o is not finite or the cell of q
 *       or of o (floor(v / resolution) per axis, a true division) leaves +-1048575.  Otherwise it is cast: the cell of q,
 *       if the map's hash has it with a cell id in range, gets hit += 1.  L = sqrt((dx*dx + dy*dy) + dz*dz).  L <=
 *       end_margin: nothing is traversed.  Otherwise s_end = 1 - end_margin / L.
 *     Traversal (Amanatides-Woo in the ray parameter s in [0, s_end)): the start cell c is the cell of o; per axis
 *       step_a = sign(d_a), tMax_a = ((c_a + (step_a > 0)) * resolution - o_a) / d_a, tDelta_a = resolution / |d_a|, and
 *       tMax_a = tDelta_a = +inf where d_a = 0.  s_in = 0.  Each step: (1) the axis of the smallest tMax, ties to the lowest
 *       axis index; (2) the current cell covers [s_in, s_out], s_out = min(tMax_axis, s_end); (3) the cell is evaluated over
 *       that segment; (4) stop if tMax_axis >= s_end; (5) stop after max_steps cells, the ray then counts as cut;
 *       (6) c_axis += step_axis, and a cell index beyond +-1048575 ends the ray (not cut); s_in = tMax_axis,
 *       tMax_axis += tDelta_axis.
 *     Evaluation: a cell that is not in the map, or whose record is not valid (a valid record has count >= 2), does
 *       nothing; the record is read only.  With A the record's inverse covariance and mu its mean: y = A d (row i as
 *       (A_i0*d0 + A_i1*d1) + A_i2*d2), a = d . y, b = y . (mu - o), s* = b / a.  If not a > 0, or s* is NaN, the ray does
 *       not pass.  Otherwise s = min(max(s*, s_in), s_out), x = (o + s*d) - mu per axis, l = x . (A x), and the ray passes
 *       iff l <= through_sigma * through_sigma (one product, on the host).  Every dot product is (u0*v0 + u1*v1) + u2*v2,
 *       every operation is rounded on its own.  A passing ray does pass[cell] += 1.
 *     Decision, per assigned cell with count > 0 and a valid record: hit >= 1 sets miss = 0; else pass >= min_pass does
 *       miss += 1 and the cell counts as seen through; else miss keeps its value.  Then miss >= miss_frames clears the
 *       cell: count = 0, the six entries of S are 0.0, the 80-byte record is all zero (valid = 0), miss = 0.  A cleared
 *       cell keeps its key, its hash entry and its cell id: capacity is NOT reclaimed.  A later sps_ndt_map_update that
 *       puts points into it takes its stored-n = 0 branch, so the refilled cell has the bits of a founded cell.  Every
 *       other cell keeps every bit, miss included.
 *   info_dev int32[4] = (rays cast, cells seen through, cells cleared, rays cut at max_steps).  The results are integer
 *   counts and comparisons of individually rounded doubles: they depend on the set of rays and the pose only, not on the
 *   order of the rays or of the threads.  Three launches whatever the data; the only atomics are integer adds.
 *   scratch_dev: sps_ndt_map_carve_scratch(cap) bytes, which is 0 (scratch_dev may be NULL; -1 for cap out of range).
 *   Never allocates, never synchronises, never raises the sticky error.
 * sps_ndt_map_carve_cells: debug -- pass, hit and miss, cell_capacity entries each (any output may be NULL).
 *   Synchronises. */
int64_t sps_ndt_map_carve_scratch(int64_t cap);
int sps_ndt_map_carve(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                      const double *T_dev, const int32_t *gate_dev, double end_margin, double through_sigma, int min_pass,
                      int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream);
int sps_ndt_map_carve_cells(sps_ctx *ctx, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev);

/* ---- NDT localiser, multi-resolution pyramid --------------------------------------------------------------------------
 * One alignment registered coarse to fine: coarse cells give a wide basin, fine cells the accuracy, and the pose is handed
 * from level to level on the device, so the host issues the same launches whatever the data does.    Additive:
 * sps_version() is unchanged, and neither the context's single map nor any call above is touched.
 *
 * sps_ndt_pyramid_build: n_levels (1 .. SPS_NDT_PYR_MAX_LEVELS) static cell maps of the same map points, coarsest first:
 *   level l groups map_xyz_dev[n_map][3] by cells of edge resolution[l] (host arrays of n_levels entries: cell_keys_dev[l],
 *   cell_start_dev[l], cell_pts_dev[l] device pointers as for sps_ndt_map_build, n_cells[l], resolution[l]).  Level l holds,
 *   bit for bit, the map sps_ndt_map_build makes from the same arguments; a level may have no cells.  Every level is checked
 *   as sps_ndt_map_build checks; resolutions must be strictly decreasing.  (-d1, d2) of the Gaussian fit is made here per
 *   level from outlier_ratio and resolution[l], as sps_ndt_align makes it per call.  The levels live in the context beside
 *   its single map; a second build replaces the first.  Allocates and synchronises.
 * sps_ndt_pyramid_cells: sps_ndt_map_cells of level `level`.
 * sps_ndt_pyramid_align: up to `iters` slots, a slot being one iteration of sps_ndt_align (launch A, launch B) against the
 *   map of the current level.  The call starts at level 0.  After a step at level l that level's count of used slots goes
 *   up by one; then
 *     |v| < tol_t and |omega| < tol_r:  on the last level status 0 and the call is done; otherwise the current level becomes
 *       l + 1 and nothing else changes: the pose carries over;
 *     else, the count has reached level_iters[l] (host int32[n_levels], each >= 1):  on the last level the call is done with
 *       status 1; otherwise the current level becomes l + 1.
 *   Fewer than min_corr points counted (status 2) and a failed Cholesky or non-finite solution (status 3) are final at any
 *   level, and T_out_dev is then T_init_host bit for bit.  Slots beyond `iters` do not exist: a call that has not reached
 *   status 0 by then has status 1, whatever level it is at.
 *   status_dev int32[4] = (code, slots used, points counted in the last live slot, level of the last live slot).
 *   trace_dev double[iters][4] and normal_dev (may be NULL) double[iters][28] are sps_ndt_align's rows, one per slot;
 *   level_dev int32[iters] is the level slot s ran at, -1 for a slot that did no work.  Per slot the operations and the
 *   order of the sums are sps_ndt_align's, so one level gives its bits and several levels give those of as many
 *   sps_ndt_align calls with iters = level_iters[l], each started from the end pose of the one before (while every one of
 *   them ends with status 0 or 1).  neighbours, cap, iters and the tolerances are checked as for sps_ndt_align.
 *   Launches: 1 + 2 * iters, no memset.  scratch_dev: sps_ndt_pyramid_align_scratch(cap) bytes (-1 for cap out of range).
 *   Never allocates, never synchronises, never raises the sticky error. */
#define SPS_NDT_PYR_MAX_LEVELS 4
int sps_ndt_pyramid_build(sps_ctx *ctx, int n_levels, const uint64_t *const *cell_keys_dev, const int32_t *const *cell_start_dev,
                          const int32_t *const *cell_pts_dev, const int64_t *n_cells, const double *resolution,
                          const double *map_xyz_dev, int64_t n_map, int min_points, double eig_ratio, double outlier_ratio,
                          void *stream);
int sps_ndt_pyramid_cells(sps_ctx *ctx, int level, uint64_t *key_out_dev, int32_t *count_out_dev, double *mean_out_dev,
                          double *icov_out_dev, int32_t *valid_out_dev);
int64_t sps_ndt_pyramid_align_scratch(int64_t cap);
int sps_ndt_pyramid_align(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host,
                          int iters, const int32_t *level_iters, int neighbours, int min_corr, double tol_t, double tol_r,
                          double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, int32_t *level_dev,
                          void *scratch_dev, void *stream);

/* ---- NDT localiser, online pyramid ------------------------------------------------------------------------------------
 * The pyramid above with the online map's two operations: every level is a dynamic map (moments, capacity, carve counters),
 * and one call updates, one call carves, all levels in the same launches, the level being a grid dimension.  
 * These are the launches of sps_ndt_map_update and sps_ndt_map_carve, whose single map is a pyramid of one level.
 * Additive: sps_version() is unchanged; the context's single map and every call above keep their behaviour and their bits.
 *
 * sps_ndt_pyramid_build_dynamic: sps_ndt_pyramid_build with cell_capacity (host int64[n_levels]).  Level l is the map that
 *   sps_ndt_map_build_dynamic makes from the same arguments at resolution[l] with cell_capacity[l]: its first n_cells[l]
 *   records, counts, keys, moments S and its state are those bits; the unassigned records are zero, their keys empty, and
 *   pass / hit / miss are zero.  Every level is checked as sps_ndt_map_build_dynamic checks (cell_capacity[l] >=
 *   max(n_cells[l], 1)).  n_map = 0 builds an empty pyramid to grow from.  Either pyramid build replaces whatever pyramid
 *   the context had; neither touches the context's single map.  Allocates and synchronises.
 *   sps_ndt_pyramid_align runs unchanged on dynamic levels (a level's n_cells is then its capacity, as for the single
 *   dynamic map), and sps_ndt_pyramid_cells(level) writes cell_capacity[level] rows.
 * sps_ndt_pyramid_update: sps_ndt_map_update on every level.  Level l ends with the bits that sps_ndt_map_update leaves on
 *   a single dynamic map of resolution[l] and cell_capacity[l] given the same points, pose, gate and max_cell_points: every
 *   byte of the records, counts, keys, S and state, and info_dev[l] (int32[n_levels][4], sps_ndt_map_update's four words per
 *   level, coarsest first).  Pose and gate rules are sps_ndt_map_update's: T_dev wins over T_host where both are given;
 *   gate_dev NULL or pointing at a status word that is 0 or 1 opens the gate (status_dev of sps_ndt_pyramid_align is a
 *   valid gate); a closed gate changes no byte of any level and gives info (assigned, 0, 0, 0) per level.  A context whose
 *   pyramid is static, or that has none, is refused with SPS_ERR_INVALID.
 *   Launches: seven and two memsets, whatever n_levels and the data.  scratch_dev: sps_ndt_pyramid_update_scratch(cap,
 *   n_levels) bytes (-1 for cap or n_levels out of range; cap <= SPS_NDT_UPDATE_MAX_POINTS), n_levels being the pyramid's.
 *   Never allocates, never synchronises, never raises the sticky error.
 * sps_ndt_pyramid_carve: sps_ndt_map_carve on every level, with end_margin a host double[n_levels] and info_dev
 *   int32[n_levels][4].  Level l ends with the pass, hit, miss, map and info that sps_ndt_map_carve leaves on the single
 *   map of that resolution with end_margin[l]; the other options are shared and checked as sps_ndt_map_carve checks them.
 *   Launches: three, no memset, whatever n_levels.  sps_ndt_pyramid_carve_scratch is 0 (-1 out of range); scratch_dev may
 *   be NULL.  Never allocates, never synchronises, never raises the sticky error.
 * sps_ndt_pyramid_info: sps_ndt_map_info of level `level` (out_host int64[4]: assigned, capacity, dropped since the build,
 *   0).  sps_ndt_pyramid_carve_cells: sps_ndt_map_carve_cells of level `level`, cell_capacity[level] entries each.  Both
 *   are debug getters and synchronise. */
int sps_ndt_pyramid_build_dynamic(sps_ctx *ctx, int n_levels, const uint64_t *const *cell_keys_dev,
                                  const int32_t *const *cell_start_dev, const int32_t *const *cell_pts_dev, const int64_t *n_cells,
                                  const double *resolution, const double *map_xyz_dev, int64_t n_map, int min_points,
                                  double eig_ratio, double outlier_ratio, const int64_t *cell_capacity, void *stream);
int64_t sps_ndt_pyramid_update_scratch(int64_t cap, int n_levels);
int sps_ndt_pyramid_update(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                           const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev,
                           void *scratch_dev, void *stream);
int64_t sps_ndt_pyramid_carve_scratch(int64_t cap, int n_levels);
int sps_ndt_pyramid_carve(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                          const double *T_dev, const int32_t *gate_dev, const double *end_margin, double through_sigma,
                          int min_pass, int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream);
int sps_ndt_pyramid_info(sps_ctx *ctx, int level, int64_t *out_host);
int sps_ndt_pyramid_carve_cells(sps_ctx *ctx, int level, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev);

/* ---- NDT localiser, pyramid, several hypotheses ------------------------------------------------------------------------
 * sps_ndt_pyramid_align from n_hyp start poses that live on the device, in the same launches, and sps_ndt_align_batch's
 * choice among the end poses.    Additive: sps_version() is unchanged, and every call above keeps its
 * behaviour and its bits.
 *
 * sps_ndt_pyramid_align_batch: hypothesis k starts from the row-major 4x4 T_init_dev[k] (the caller leaves it unchanged
 *   until the stream has passed the call; work issued earlier on the stream may still be writing it) and is, operation for
 *   operation and sum for sum, sps_ndt_pyramid_align from that pose: T_out_dev[k], status_dev[k] (int32[n_hyp][4]: code,
 *   slots used, points counted in the last live slot, its level), trace_dev[k] (double[n_hyp][iters][4]), normal_dev[k]
 *   (may be NULL; double[n_hyp][iters][28]) and level_dev[k] (int32[n_hyp][iters]) have the bits of the single call, the
 *   zero rows and the -1 levels of slots that did no work included, and T_out_dev[k] is T_init_dev[k] bit for bit on status
 *   2 and 3.  Every hypothesis has state words of its own in the scratch (done, level, slots used per level): hypotheses
 *   stand at different levels in the same slot, and one whose status is final sits out the remaining slots while the others
 *   go on.  The scan points and the levels are shared.  With a pyramid of one level every output, final_dev, best_dev and
 *   T_best_dev included, has the bits of sps_ndt_align_batch on a single map of that resolution.
 *   Launches: 1 (initialise: poses, statuses, state words and the per-slot rows) + 2 * iters (A with grid
 *   (ceil(cap / 32), n_hyp), B with grid n_hyp) + 2, whatever the data, no memset:
 *     A once more, sps_ndt_align_batch's body, for every hypothesis at its final pose whatever its status, against the map
 *        and the Gaussian fit of the finest level (so the scores compare however far a hypothesis got): final_dev[k] = (score,
 *        points counted), the partial rows added in launch B's block order;
 *     select, sps_ndt_align_batch's: the highest final score among the hypotheses with status 0 or 1 (one that used up
 *        `iters` on a coarse level is eligible) and at least min_corr points counted at the final pose; equal scores go to
 *        the lowest k; NaN never wins.  best_dev = (k, status of k, points counted at its final pose, n_hyp) and T_best_dev
 *        = T_out_dev[k]; where no hypothesis qualifies best_dev = (-1, -1, 0, n_hyp) and T_best_dev = T_init_dev[0].
 *   iters = 0 is legal: final_dev[k] is then what sps_ndt_score_poses gives for T_init_dev[k] on a single map of the finest
 *   resolution.  T_best_dev and best_dev + 1 serve as T_dev and gate_dev of sps_ndt_pyramid_update / sps_ndt_pyramid_carve.
 *   Arguments are checked as for sps_ndt_pyramid_align (level_iters: host int32[n_levels], each >= 1), and 1 <= n_hyp <=
 *   SPS_NDT_MAX_HYP.  A context without a pyramid is refused with SPS_ERR_INVALID; a static and a dynamic pyramid are both
 *   accepted.  scratch_dev: sps_ndt_pyramid_align_batch_scratch(cap, n_hyp) bytes, the partial rows of every hypothesis
 *   and then NDT_PYR_STATE = 8 state words each (-1 for arguments out of range).  Never allocates, never synchronises, never
 *   raises the sticky error. */
int64_t sps_ndt_pyramid_align_batch_scratch(int64_t cap, int n_hyp);
int sps_ndt_pyramid_align_batch(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_dev,
                                int n_hyp, int iters, const int32_t *level_iters, int neighbours, int min_corr, double tol_t,
                                double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev,
                                int32_t *level_dev, double *final_dev, int32_t *best_dev, double *T_best_dev, void *scratch_dev,
                                void *stream);

/* ---- NDT localiser, distribution to distribution ------------------------------------------------------------------------
 * hdl_localization's other registration family (reg_method NDT_CUDA_D2D / VGICP): the scan is reduced to Gaussians too, one
 * per cell of the sensor frame, and Gaussians are registered against Gaussians.    Additive: sps_version()
 * is unchanged.  The rules of sps_ndt_align hold (float64, every operation rounded on its own, no float atomics, no sum
 * whose order depends on thread arrival); neither call allocates, synchronises or raises the sticky error.
 *
 * sps_ndt_source_build: pts_dev is sps_loc_downsample's output (f64 [cap][3], sensor frame), of which the first
 *   min(cap, *n_dev) rows are used; cap <= SPS_NDT_UPDATE_MAX_POINTS.
 *   - The cell of a point is floor(p / source_resolution) per axis (a true division, as the map's); a non-finite coordinate
 *     or a cell index beyond +-1048575 skips the point.
 *   - Source cell j is the j-th cell in ascending order of the lowest point index that falls in it (the founder rule of
 *     sps_ndt_map_update).
 *   - Per cell: n, mean = (sum of the points in ascending point index) / n, S = sum (p - mean)(p - mean)^T in the same
 *     order (the operation order of sps_ndt_map_build: sum, divide, second pass of outer products).
 *   - Record, SPS_NDT_SRC_REC doubles: mean[3], covariance[6] (xx, xy, xz, yy, yz, zz), valid (1.0 / 0.0).  The covariance
 *     is S / (n - 1), decomposed by the 8 cyclic Jacobi sweeps of the map, its eigenvalues floored at eig_ratio * lambda_max,
 *     and reassembled, entry (i, j) = ((v_i0 v_j0) l0 + (v_i1 v_j1) l1) + (v_i2 v_j2) l2; zero for n < 2.
 *   - Valid iff n >= min_points, n >= 2, lambda_max > 0 and every number of the record is finite.  Invalid cells keep their
 *     slot, flagged.
 *   - n_src_dev = (cells, valid cells).  src_count_dev (may be NULL): n per cell.  Rows of src_dev and src_count_dev beyond
 *     the cells are not written.  *n_dev = 0 gives (0, 0); cap = 0 is legal.
 *   The grouping is the online update's: its kernels' bodies run against an empty map of capacity `cap` in the scratch, at
 *   the identity pose.  Launches: seven and four memsets, whatever the data.  scratch_dev: sps_ndt_source_scratch(cap)
 *   bytes (-1 for cap out of range), 256-byte aligned.
 *
 * sps_ndt_align_d2d: sps_ndt_align with launch A replaced; launch B, the partial rows (one per 32 sources), the outputs,
 *   the status codes, "T_out = T_init bit for bit on 2 / 3" and the checks of the arguments are sps_ndt_align's.  It runs
 *   against the map of the context, static or online; d1 and d2 come from outlier_ratio and the MAP's resolution.
 *   src_dev [cap_src][SPS_NDT_SRC_REC] and n_src_dev are sps_ndt_source_build's (or hand-made); the first
 *   min(cap_src, n_src_dev[0]) records are read and the valid ones used.
 *   Launch A, per valid source (mu, C) at the pose (R, t):
 *     q = R mu + t, per axis ((R0 mu0 + R1 mu1) + R2 mu2) + t;
 *     Cw = R C R^T: U = R C first, every entry (a0 b0 + a1 b1) + a2 b2, then Cw = U R^T the same way;
 *     cells: q's own, then +x, -x, +y, -y, +z, -z (neighbours = 7) or q's own (1), by the map's cell rule;
 *     per valid map record (mean m, inverse covariance A): Sm = inv3(A), M = Sm + Cw entry by entry, B = inv3(M),
 *       x = q - m, y = B x (rows as (B0 x0 + B1 x1) + B2 x2), s = (x0 y0 + x1 y1) + x2 y2, e = exp(-0.5 (d2 s)), w = d2 e;
 *       the cell is skipped unless 0 <= w <= 1 (NaN skips), and if either inv3 met det <= 0 or a non-finite entry;
 *     inv3 of (m0 .. m5) = (xx, xy, xz, yy, yz, zz): c00 = m3 m5 - m4 m4, c01 = m2 m4 - m1 m5, c02 = m1 m4 - m2 m3,
 *       c11 = m0 m5 - m2 m2, c12 = m1 m2 - m0 m4, c22 = m0 m3 - m1 m1, det = (m0 c00 + m1 c01) + m2 c02, every entry
 *       c / det by a true division;
 *     with a = (-d1) w and J = [-[q]x | I] at q: H(r, c) += a (J_r . (B J_c)), g(r) += a (J_r . y), score += (-d1) e; a
 *       source with at least one contributing cell counts once.
 *   Orders: cells in lookup order within a source, sources in index order within a workgroup of 32, workgroups as launch B
 *   adds them.  The step is the house's: B is held at the current pose (its dependence on R is not differentiated), H is
 *   the positive-semidefinite part only, H delta = -g is taken at unit length, and sources are not weighted by their point
 *   counts.  Status 2: fewer than min_corr SOURCES counted.  trace_dev = (sources counted, score, |v|, |omega|) per
 *   iteration.  The map keeps its layout: its covariance is recovered from the record's inverse covariance, whose
 *   condition number the eigenvalue floor keeps <= 1 / eig_ratio.  Launches: 1 + 2 * iters and up to two memsets.
 *   scratch_dev: sps_ndt_align_d2d_scratch(cap_src) bytes (-1 for cap_src out of range). */
#define SPS_NDT_SRC_REC 10
int64_t sps_ndt_source_scratch(int64_t cap);
int sps_ndt_source_build(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, double source_resolution,
                         int min_points, double eig_ratio, double *src_dev, int32_t *src_count_dev, int32_t *n_src_dev,
                         void *scratch_dev, void *stream);
int64_t sps_ndt_align_d2d_scratch(int64_t cap_src);
int sps_ndt_align_d2d(sps_ctx *ctx, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                      const double *T_init_host, int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t,
                      double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev,
                      void *scratch_dev, void *stream);

/* ---- NDT localiser, distribution to distribution, several poses ---------------------------------------------------------
 * What "several hypotheses" and "pose search" above give the point registration, for source cells: sps_ndt_align_d2d from
 * n_hyp start poses that live on the device, with best-score selection, and the D2D score of a grid of poses.  (DESIGN.md
 * 8o.)  Additive: sps_version() is unchanged.  The rules of sps_ndt_align_d2d hold; src_dev, n_src_dev and cap_src are its
 * arguments, and the first min(cap_src, n_src_dev[0]) records are read and the valid ones used.  Static and online maps are
 * both accepted.  No call allocates, synchronises or raises the sticky error.
 *
 * sps_ndt_align_d2d_batch: hypothesis k starts from the row-major 4x4 T_init_dev[k] (double[n_hyp][16] on the device, which
 *   work issued earlier on the stream may still be writing; the caller leaves it unchanged until the stream has passed the
 *   call) and is, operation for operation and sum for sum, sps_ndt_align_d2d from that pose: T_out_dev[k], status_dev[k],
 *   trace_dev[k] and normal_dev[k] have the bits of the single call, T_out_dev[k] is T_init_dev[k] bit for bit on status 2
 *   and 3, and a hypothesis whose status is final sits out the remaining iterations while the others go on.  The source
 *   records and the map are shared.  iters = 0 is legal.
 *   Launches: 1 (initialise) + 2 * iters (A with grid (ceil(cap_src / 32), n_hyp), B with grid n_hyp) + 2, whatever the
 *   data, and the up to two memsets of the single call (trace_dev, normal_dev; none with iters = 0):
 *     A once more, for every hypothesis at its final pose whatever its status: final_dev[k] = (D2D score at the final pose,
 *        sources counted), the partial rows (one per 32 sources) added in launch B's block order;
 *     select (sps_ndt_align_batch's): the hypothesis with the highest final score among those with status 0 or 1 and at
 *        least min_corr sources counted at the final pose; equal scores go to the lowest k, NaN never wins.  best_dev = (k,
 *        status of k, sources counted at its final pose, n_hyp) and T_best_dev = T_out_dev[k]; where no hypothesis
 *        qualifies best_dev = (-1, -1, 0, n_hyp) and T_best_dev = T_init_dev[0].
 *   T_best_dev and best_dev + 1 serve as T_dev and gate_dev of sps_ndt_map_update, sps_ndt_map_carve, sps_loc_match_status
 *   and sps_ukf_correct.  Arguments are checked as for sps_ndt_align_d2d, and 1 <= n_hyp <= SPS_NDT_MAX_HYP.  trace_dev
 *   double[n_hyp][iters][4], normal_dev (may be NULL) double[n_hyp][iters][28].  scratch_dev:
 *   sps_ndt_align_d2d_batch_scratch(cap_src, n_hyp) bytes (-1 for arguments out of range): the partial rows of every
 *   hypothesis, then one done flag each.
 *
 * sps_ndt_score_poses_d2d: score_dev[p] = (D2D score, sources counted) of the row-major 4x4 pose T_dev[p].  Per valid
 *   source and pose this is launch A of sps_ndt_align_d2d restricted to its last two sums: q = R mu + t and Cw = R C R^T as
 *   there, the cells of q in lookup order, per valid map record Sm, M, B, x, y, s, e and w as there with the same guards,
 *   score += (-d1) e, and a source with at least one contributing cell counts once.  Orders: cells in lookup order within a
 *   source, sources in index order within a workgroup of 32, workgroups as launch B adds them.  score_dev[p] therefore has
 *   the bits of final_dev[k] of sps_ndt_align_d2d_batch(iters = 0) started at T_dev[p].  A pose with a NaN entry, or one
 *   that puts every source off the map, scores (0, 0).  An empty map, n_src_dev[0] = 0 and records that are all invalid are
 *   legal: every pose scores (0, 0).  1 <= n_pose <= SPS_NDT_MAX_POSES; neighbours, outlier_ratio and cap_src are checked
 *   as for sps_ndt_align_d2d.  Launches: 2 per chunk of poses (the scorer with grid (ceil(cap_src / 32), ceil(poses of
 *   the chunk / 32)), then the reduction of sps_ndt_score_poses).  scratch_dev: sps_ndt_score_d2d_scratch(cap_src, n_pose)
 *   bytes (-1 for arguments out of range) = 16 * ceil(cap_src / 32) bytes per pose of a chunk, chunked under the bound of
 *   sps_ndt_score_scratch: at or below 64 MiB, or the 32 poses of one tile where those need more.  sps_ndt_top_poses
 *   serves unchanged on score_dev, min_corr then meaning sources.  T_dev stays unchanged until the stream has passed the
 *   call. */
int64_t sps_ndt_align_d2d_batch_scratch(int64_t cap_src, int n_hyp);
int sps_ndt_align_d2d_batch(sps_ctx *ctx, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                            const double *T_init_dev, int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio,
                            double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                            double *normal_dev, double *final_dev, int32_t *best_dev, double *T_best_dev, void *scratch_dev,
                            void *stream);
int64_t sps_ndt_score_d2d_scratch(int64_t cap_src, int64_t n_pose);
int sps_ndt_score_poses_d2d(sps_ctx *ctx, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_dev,
                            int64_t n_pose, int neighbours, double outlier_ratio, double *score_dev, void *scratch_dev,
                            void *stream);

/* ---- NDT localiser, distribution to distribution, pyramid ----------------------------------------------------------------
 * sps_ndt_align_d2d registered coarse to fine: the scan's cells are built at one resolution per level and registered against
 * the context's pyramid of map cells, the pose handed from level to level on the device as sps_ndt_pyramid_align hands it.
 *   Additive: sps_version() is unchanged, and no call above changes.  The rules of sps_ndt_align_d2d hold;
 * neither call allocates, synchronises or raises the sticky error.
 *
 * sps_ndt_pyramid_source_build: sps_ndt_source_build at n_levels (1 .. SPS_NDT_PYR_MAX_LEVELS) resolutions at once.
 *   source_resolution and min_points are host arrays of n_levels entries, in no way tied to the map's levels (equal entries
 *   are legal).  src_dev double[n_levels][cap][SPS_NDT_SRC_REC], src_count_dev int32[n_levels][cap] (may be NULL) and
 *   n_src_dev int32[n_levels][2]: level l is, bit for bit, what sps_ndt_source_build writes for (source_resolution[l],
 *   min_points[l]): records, counts, (cells, valid cells), and the rows beyond the cells are not written.  It does not read
 *   the context's maps.  Arguments are checked as sps_ndt_source_build checks them, every level's.  Launches: seven and four
 *   memsets whatever n_levels and the data (the level is a grid dimension).  scratch_dev:
 *   sps_ndt_pyramid_source_scratch(cap, n_levels) bytes (-1 for arguments out of range), 256-byte aligned.
 *
 * sps_ndt_pyramid_align_d2d: sps_ndt_pyramid_align with launch A replaced by sps_ndt_align_d2d's, against the pyramid of
 *   sps_ndt_pyramid_build[_dynamic] (refused without one).  src_dev and n_src_dev are sps_ndt_pyramid_source_build's (or
 *   hand-made) with cap = cap_src and n_levels = the pyramid's: a slot at level l reads the first min(cap_src, n_src_dev[l][0])
 *   records of src_dev[l] against the map of level l, with that level's (-d1, d2).  Slots, level_iters, status_dev (its third
 *   word counts sources), trace_dev, normal_dev, level_dev, the budget and "status 2 / 3 are final at any level and T_out_dev
 *   is then T_init_host bit for bit" are sps_ndt_pyramid_align's.  The handoff has one more rule: the call starts at level 0,
 *   and the level that follows l is the next l' > l whose valid sources, min(cap_src, n_src_dev[l'][1]), are at least
 *   min_corr; where there is none, l is the last level: its convergence is status 0 and its cap ends the call with status 1.
 *   (A level with fewer valid sources could only end the call with status 2 and throw the pose away.)  So one level gives
 *   the bits of sps_ndt_align_d2d, and several levels those of as many sps_ndt_align_d2d calls with iters = level_iters[l]
 *   over the levels entered, each started from the end pose of the one before (while every one of them ends with status 0
 *   or 1).  Launches: 1 + 2 * iters, no memset.  scratch_dev: sps_ndt_pyramid_align_d2d_scratch(cap_src) bytes (-1 for
 *   cap_src out of range). */
int64_t sps_ndt_pyramid_source_scratch(int64_t cap, int n_levels);
int sps_ndt_pyramid_source_build(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, int n_levels,
                                 const double *source_resolution, const int32_t *min_points, double eig_ratio, double *src_dev,
                                 int32_t *src_count_dev, int32_t *n_src_dev, void *scratch_dev, void *stream);
int64_t sps_ndt_pyramid_align_d2d_scratch(int64_t cap_src);
int sps_ndt_pyramid_align_d2d(sps_ctx *ctx, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                              const double *T_init_host, int iters, const int32_t *level_iters, int neighbours, int min_corr,
                              double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                              double *normal_dev, int32_t *level_dev, void *scratch_dev, void *stream);

/* ---- NDT localiser, distribution to distribution, pyramid, several hypotheses ---------------------------------------------
 * sps_ndt_pyramid_align_d2d from n_hyp start poses that live on the device, in the same launches, and
 * sps_ndt_align_batch's choice among the end poses.    Additive: sps_version() is unchanged, and no call
 * above changes its bits or its behaviour.  The rules of sps_ndt_align_d2d hold; the call does not allocate, does not
 * synchronise and never raises the sticky error.
 *
 * sps_ndt_pyramid_align_d2d_batch: src_dev double[n_levels][cap_src][SPS_NDT_SRC_REC] and n_src_dev int32[n_levels][2]
 *   (cells, valid cells) are sps_ndt_pyramid_source_build's (or hand-made), the levels back to back.  Every other argument
 *   and output means what it means in sps_ndt_pyramid_align_batch.  Hypothesis k is, operation for operation and sum for
 *   sum, sps_ndt_pyramid_align_d2d from T_init_dev[k]: T_out_dev[k], status_dev[k], its trace, normal and level rows and
 *   the slots used per level have the bits of the single call.  Hypotheses stand at different levels in the same slot: launch
 *   A of hypothesis k reads the map, the source records and the count of the level its state words name, launch B sums the
 *   rows of that level's count and hands off by sps_ndt_pyramid_align_d2d's skip rule.  The sources are in the sensor
 *   frame, so every hypothesis walks the same chain of levels.
 *   Launches: 1 + 2 * iters + 2, whatever the data, no memset:
 *     the final pass: the scoring level l* is the last level of that chain, the largest l >= 1 with
 *        min(cap_src, n_src_dev[l][1]) >= min_corr, or 0 where there is none.  It is found on the device; the host never
 *        reads it during the call.  Every hypothesis, whatever its status and the level it stopped at, is evaluated at
 *        T_out_dev[k] with level l*'s sources against level l*'s map: final_dev[k] = (D2D score, sources counted), the bits of
 *        sps_ndt_score_poses_d2d at T_out_dev[k] on a single map and single sources built at level l*'s two resolutions and
 *        min_points.  A finest level that was skipped is not used for scoring.
 *     select, sps_ndt_align_batch's, on the rows of level l*'s count: the highest score among status 0 or 1 with at least
 *        min_corr sources counted; ties go to the lowest k; NaN never wins.  best_dev = (k, status of k, sources counted at
 *        its final pose, n_hyp), T_best_dev = T_out_dev[k]; nobody qualifies: (-1, -1, 0, n_hyp) and T_init_dev[0].
 *   Level 0 with fewer than min_corr sources counted is status 2 for every hypothesis after one slot.  iters = 0 is legal
 *   and gives the scores of the start poses.  Arguments are checked as for sps_ndt_pyramid_align_batch and
 *   sps_ndt_pyramid_align_d2d: 1 <= n_hyp <= SPS_NDT_MAX_HYP, a built pyramid, level_iters each >= 1, the limits on cap_src.
 *   scratch_dev: sps_ndt_pyramid_align_d2d_batch_scratch(cap_src, n_hyp) bytes (-1 for arguments out of range): the layout
 *   of sps_ndt_pyramid_align_batch_scratch with the source capacity.  The final pass leaves (count of level l*, l*) in the
 *   two spare state words of hypothesis 0. */
int64_t sps_ndt_pyramid_align_d2d_batch_scratch(int64_t cap_src, int n_hyp);
int sps_ndt_pyramid_align_d2d_batch(sps_ctx *ctx, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                                    const double *T_init_dev, int n_hyp, int iters, const int32_t *level_iters, int neighbours,
                                    int min_corr, double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev,
                                    double *trace_dev, double *normal_dev, int32_t *level_dev, double *final_dev,
                                    int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream);

/* ---- pose estimator (unscented Kalman filter with IMU prediction) -----------------------------------------------------
 * hdl_localization's pose system as published, restated: tests/ukf_reference.py is the specification, not that package
 * (DESIGN.md 8j lists the differences).  Additive: sps_version() is unchanged.  No entry takes a context, allocates,
 * synchronises or raises a sticky error; each is one launch of one workgroup on `stream`.
 *
 * State (n = 16, f64): p 0:3, v 3:6, q 6:10 (w, x, y, z), accelerometer bias 10:13, gyroscope bias 13:16.  The state
 * block is a caller-owned device buffer of SPS_UKF_STATE_BYTES: x[16] | P[16][16] (row-major, exactly symmetric) |
 * T[16] (the pose of the mean) | int32 (predictions done, corrections done, 0, 0).
 *
 * Process f(x, (a, w), dt): p' = p + v dt; v' = v (the acceleration is accepted in every sample and unused); g = w - bg,
 *   h = (dt / 2) g, dq = (1, h) / |(1, h)|, q' = (q * dq) / |q * dq| (Hamilton product, body-frame rate); biases unchanged.
 *   Without an IMU g = 0 and q' = q / |q|.
 * Prediction: unscented transform with lambda = 1: L = chol(17 P), 33 sigma points x, x + L[:, i], x - L[:, i], weights
 *   1/17 and 1/34, all through f; mean = sum w_i s_i; P = sum w_i (s_i - mean)(s_i - mean)^T + diag(process_diag) dt; then
 *   the mean's quaternion is renormalised.
 * Correction with z = (p, q) of a 4 x 4 pose (q by Shepperd's method: the largest of trace, R00, R11, R22 decides, ties to
 *   the first; normalised; negated where its dot product with the mean's quaternion is negative): the state is extended by
 *   the measurement noise (23 entries, 47 sigma points, weights 1/24 and 1/48); the extended covariance is block diagonal,
 *   so its factor is chol(24 P) and sqrt(24 r_k).  z_i = (p_i, q_i) + noise_i, zbar = sum w_i z_i, Pz = sum w_i dz dz^T,
 *   Pxz = sum w_i (s_i - x) dz^T, K = Pxz Pz^-1 through chol(Pz) and two triangular solves per row, x += K (z - zbar),
 *   P -= (K Pz) K^T, the mean's quaternion renormalised.
 * Arithmetic: every operation an individually rounded f64 one, no transcendental function, no float atomic; sigma points
 *   summed in index order, Cholesky and substitution inner sums in ascending index, every entry by one thread; P and Pz
 *   are computed on the lower triangle and mirrored.  Same input, same bits, whatever the launch geometry.
 * Status (int32): 0 done; 2 the gate was closed (the state block is untouched, every byte); 3 singular: a Cholesky pivot
 *   <= 0 or anything not finite -- the state is as before the failing step.
 *
 * sps_ukf_init: the state from a host pose T_host[16], a host velocity v_host[3] (NULL: zero) and the diagonal of P
 *   (p0_diag[16], finite, >= 0); the counters are cleared.
 * sps_ukf_predict: imu_dev is [n_imu][7] f64 rows (dt, ax, ay, az, gx, gy, gz), 0 <= n_imu <= SPS_UKF_MAX_IMU: one launch
 *   runs every sample in turn.  n_imu = 0 only writes the pose.  T_pred_dev (may be NULL) receives the pose of the mean
 *   after the call, info_dev (may be NULL) int32 (status, samples done, index of the failing sample or -1, 0).  A sample
 *   that is not finite, whose dt is not > 0, or whose step is singular ends the call with status 3: the state is that of
 *   the sample before it and the remaining samples are skipped.  process_diag_host: double[16], finite, >= 0.
 * sps_ukf_predict_dt: the IMU-less step over dt (finite, > 0, checked before anything is queued), on the same kernel.
 * sps_ukf_correct: T_meas_dev is a 4 x 4 pose on the device (T_out of an alignment, T_best of a batch); gate_dev (NULL:
 *   always correct) an int32 on the device: the correction runs where it is 0 or 1 (the status word of an alignment,
 *   best[1] of a batch: the gate of sps_ndt_map_update and sps_ndt_map_carve).  meas_diag_host: double[7], finite, >= 0.
 *   info_dev (may be NULL): 8 doubles, the first one's two int32 halves (status, 0), then the innovation z - zbar[7]
 *   (zeros unless the status is 0). */
#define SPS_UKF_STATE_BYTES 2320
#define SPS_UKF_MAX_IMU 256
int64_t sps_ukf_state_bytes(void);
int sps_ukf_init(double *state_dev, const double *T_host, const double *v_host, const double *p0_diag, void *stream);
int sps_ukf_predict(double *state_dev, const double *imu_dev, int32_t n_imu, const double *process_diag_host, double *T_pred_dev,
                    int32_t *info_dev, void *stream);
int sps_ukf_predict_dt(double *state_dev, double dt, const double *process_diag_host, double *T_pred_dev, int32_t *info_dev,
                       void *stream);
int sps_ukf_correct(double *state_dev, const double *T_meas_dev, const int32_t *gate_dev, const double *meas_diag_host,
                    double *info_dev, void *stream);

/* ---- NDT localiser, global search -------------------------------------------------------------------------------------
 * Where on the map is the robot, with no start pose: a branch and bound over (x, y, yaw) on a pyramid of 2-D occupancy
 * grids cut from a height slice of the map (the BBS engine of hdl_global_localization; Cartographer's fast correlative scan
 * matcher is the same method).  It ends in K start poses on the device, which sps_ndt_align_batch takes as they are.
 *   Additive: sps_version() is unchanged and no call above is touched.
 *
 * Grid: G0[H][W] bytes, 0 or 1, made by the caller; cell (i, j) covers [r (i0 + i), r (i0 + i + 1)) x [r (j0 + j), ...) of
 *   the map frame.  G_l(x, y) = max G0[y + dj][x + di] over 0 <= di, dj < 2^l, l = 0 .. levels, reads outside G0 giving 0;
 *   it is defined, and may be 1, from x, y = -(2^l - 1) on.
 * sps_bbs_map_build: copies G0 (g0_dev, a device array) and pools levels 1 .. levels on the device; the pyramid lives in
 *   the context, a second build replaces the first.  0 <= levels < SPS_BBS_MAX_LEVELS; W, H >= 1 and W + 2^levels - 1,
 *   H + 2^levels - 1 <= 16384, else INVALID.  Allocates and synchronises.
 * sps_bbs_map_level: debug -- level `level` as stored, (H + pad) rows of (W + pad) bytes with pad = 2^levels - 1 and
 *   G_level(x, y) at [y + pad][x + pad].  Synchronises.
 * sps_bbs_search: pts_dev, n_dev and cap are the thinned points of sps_loc_downsample (sensor frame), cap <= 65536.
 *   Scan: q = ((r0*x + r1*y) + r2*z) + t of T_up_host (4 x 4, finite: roll, pitch and height, which a planar search cannot
 *     find); a point is kept iff scan_z_lo <= q_z <= scan_z_hi (NaN fails).
 *   Yaws: yaw_cs_dev is double[n_yaw][2] = (cos, sin)(2 pi a / n_yaw), made by the caller; the device calls no sin or cos.
 *     u = c*q_x - s*q_y, v = s*q_x + c*q_y, dx = floor(u / resolution), dy = floor(v / resolution) (true divisions); a point
 *     whose u / resolution or v / resolution is not finite or exceeds 2^20 in magnitude contributes nothing at that yaw.
 *   Score of node (a, j, i) at level l: the sum over the kept points of G_l(i + dx, j + dy), an int32: an upper bound on
 *     every leaf below the node, at l = 0 the leaf's score.
 *   Search: the candidates of level `levels` are all (a, j, i) with j, i multiples of 2^levels inside the grid, ascending;
 *     more than 4 * frontier of them is INVALID.  Per level, downwards: every candidate is scored; those with score <
 *     min_score (>= 0) are dropped; if more than `frontier` remain, the `frontier` first by (score descending, position in
 *     the candidate list ascending) are kept; dropped_bound (from -1) becomes the maximum of itself and the highest score
 *     dropped, n_dropped grows by the number dropped; above level 0 the kept nodes, in candidate order, emit their children
 *     (i + di h, j + dj h), h = 2^(l-1), (dj, di) = (0,0), (0,1), (1,0), (1,1), those with i >= W or j >= H skipped.
 *   Result: the leaves kept at level 0 by (score descending, id ascending), id = (a * H + j) * W + i (n_yaw * H * W must fit
 *     int32, else INVALID).  top_index_dev[k], top_score_dev[k]: id and score of the first k <= SPS_NDT_MAX_HYP; T_top_dev
 *     [k][16]: their poses Trans(r (i0 + i), r (j0 + j), 0) Rz(yaw a) T_up -- entry (0, c) = c*U0c - s*U1c, entry (1, c) =
 *     s*U0c + c*U1c, the translation r * (i0 + i) resp. r * (j0 + j) added to column 3, rows 2 and 3 those of T_up, every
 *     operation rounded on its own.  Slots past the last leaf: index -1, score 0 and the pose of slot 0 (T_up where there
 *     is none).  n_top_dev: the slots filled.
 *   info_dev int32[SPS_BBS_INFO_WORDS] = (certified, dropped_bound, n_dropped, points in the slice, then per level l =
 *     0 .. 7 (candidates, kept)); certified = the leading results with score > dropped_bound: that prefix is the prefix of
 *     the exhaustive ranking of all leaves with score >= min_score.
 *   trace_dev (debug, may be NULL): int32[levels + 1][5 * frontier], per level its candidate slots [4 * frontier] (four
 *     per kept parent, -1 for a child outside the grid; level `levels`: the candidates themselves), then its kept nodes
 *     [frontier], as ids; only the entries in use are written.
 *   Launches: 2 + 4 * (levels + 1) and two memsets, whatever the data; grids are sized by capacity.  Scores are integer
 *   counts: the results do not depend on the order of points or threads.  The only atomics are integer adds.
 *   scratch_dev: sps_bbs_search_scratch(cap, n_yaw, frontier) bytes (-1 for cap > 65536, n_yaw outside [1,
 *   SPS_BBS_MAX_YAWS] or frontier outside [1, SPS_BBS_MAX_FRONTIER]).  Never allocates, never synchronises, never raises
 *   the sticky error. */
#define SPS_BBS_MAX_LEVELS 8
#define SPS_BBS_MAX_YAWS 4096
#define SPS_BBS_MAX_FRONTIER 65536
#define SPS_BBS_INFO_WORDS 20
int sps_bbs_map_build(sps_ctx *ctx, const uint8_t *g0_dev, int64_t W, int64_t H, int levels, void *stream);
int sps_bbs_map_level(sps_ctx *ctx, int level, uint8_t *out_dev);
int64_t sps_bbs_search_scratch(int64_t cap, int64_t n_yaw, int64_t frontier);
int sps_bbs_search(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_up_host,
                   double resolution, int64_t i0, int64_t j0, double scan_z_lo, double scan_z_hi, const double *yaw_cs_dev,
                   int64_t n_yaw, int64_t frontier, int min_score, int k, int32_t *top_index_dev, int32_t *top_score_dev,
                   double *T_top_dev, int32_t *n_top_dev, int32_t *info_dev, int32_t *trace_dev, void *scratch_dev,
                   void *stream);

/* ---- localiser, scan-matching status ------------------------------------------------------------------------------------
 * How well does a scan fit the map at a pose: the share of its points with a map point nearby, and their mean squared
 * distance.  A registration that converges to the wrong place ends with status 0 or 1 like a good one; this measure tells
 * them apart, on the device, and its verdict word can stand where the registration's status gates what follows it
 * (sps_ndt_map_update, sps_ndt_map_carve, sps_ukf_correct: all open on (unsigned)word <= 1).    Additive:
 * sps_version() is unchanged and no call above is touched.
 *
 * sps_loc_match_status: pts_dev, n_dev and cap are the thinned points of sps_loc_downsample (sensor frame); T_dev is a
 *   row-major 4 x 4 on the device (the T_out of an alignment, the T_best of a batch, a pose estimator's pose ...), of which
 *   the first 12 entries are read.  The map is the context's radius grid (sps_radius_grid_upload): INVALID when none was
 *   uploaded, and when max_distance is not finite and > 0 or exceeds the grid's cell size (the 27-cell search is exact
 *   only up to one cell).  NaN thresholds, min_valid < 0 and cap > SPS_MAX_POINTS are INVALID too.
 *   n = min(cap, max(*n_dev, 0)).  Point i < n is valid iff its three coordinates are finite and either max_range < 0 or
 *     (px*px + py*py) + pz*pz <= max_range*max_range (the sensor frame; the host squares both radii in float64).
 *   q = R p + t as in sps_loc_align; the nearest map point over the 27 cells around q exactly as sps_loc_align takes it:
 *     d2 = (ex*ex + ey*ey) + ez*ez, ties to the lowest map index; q not finite or outside the key range: no neighbour.
 *   A valid point is an inlier iff it has a neighbour with d2 <= max_distance^2.
 *   Each workgroup of 32 points adds its inliers' d2 in point order; a second launch with one workgroup adds the rows of
 *     the ceil(n / 32) workgroups that hold points as launch B of sps_loc_align adds its partial rows (8 runs of
 *     consecutive rows, each in order, then the runs in order).  Counts are integers.  No float atomics; nothing depends
 *     on the order in which threads arrive, so two calls give the same bits.
 *   out_dev: double[4] = (inlier_fraction, matching_error, sum_d2, 0), then int32[4] = (verdict, n_valid, n_inliers, n).
 *     inlier_fraction = n_inliers / max(n_valid, 1); matching_error = sum_d2 / n_inliers, +inf without inliers (true
 *     divisions).  verdict: g = gate_in_dev ? *gate_in_dev : 0; (unsigned)g > 1: g (the registration already failed; -1
 *     stays -1); else g where n_valid >= min_valid && inlier_fraction >= min_inlier_fraction && matching_error <=
 *     max_error; else SPS_LOC_LOST.
 *   d2_dev (may be NULL) double[cap]: the inlier's d2; +inf for a valid point that is not an inlier; -1 for a point that is
 *     not valid; rows >= n are not written.
 *   Two launches, whatever the data.  scratch_dev: sps_loc_match_status_scratch(cap) bytes (-1 for cap outside [0,
 *   SPS_MAX_POINTS]).  Never allocates, never synchronises, never raises the sticky error. */
#define SPS_LOC_LOST 4
int64_t sps_loc_match_status_scratch(int64_t cap);
int sps_loc_match_status(sps_ctx *ctx, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_dev,
                         const int32_t *gate_in_dev, double max_distance, double max_range, double min_inlier_fraction,
                         double max_error, int min_valid, double *out_dev, double *d2_dev, void *scratch_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPS_HIP_H */
