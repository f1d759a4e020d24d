/*
 * pose6d — C ABI of the MI355X (gfx950) hot path of SFR-Vision/6d-pose-estimation.
 *
 * The reference exposes this path as Python classes (models/pose_net_*.py,
 * models/pose_loss.py, models/add_loss.py); this library is what those classes'
 * forward()/backward() call in the build.  Each entry point names the reference
 * code it replaces (path:line in the reference tree).
 *
 * Conventions (all entry points):
 *  - plain device pointers + sizes; no torch types; no allocation inside: the
 *    caller passes every output and workspace buffer (sizes documented or
 *    queried with the *_workspace() functions);
 *  - `stream` is a hipStream_t (torch's current stream); every call is
 *    stream-ordered and graph-capturable (no sync, no malloc);
 *  - return 0 on success or a POSE6D_E* code; pose6d_last_error() then holds a
 *    message (thread-local);
 *  - activations are NHWC, dtype given by a POSE6D_DT_* code; parameters and
 *    statistics are fp32; conv weights for the kernels are packed OHWI
 *    (K-contiguous per output channel), see pose6d_pack_conv_weight().
 */
#ifndef POSE6D_H
#define POSE6D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POSE6D_OK 0
#define POSE6D_EINVAL 1
#define POSE6D_ELAUNCH 2
#define POSE6D_EUNSUPPORTED 3

#define POSE6D_DT_F32 0
#define POSE6D_DT_BF16 1

int pose6d_version(void);
const char *pose6d_last_error(void);

/* ------------------------------------------------------------------------
 * ADD / ADD-S evaluation — replaces ADDLoss.eval_metrics (add_loss.py:156-201)
 * and ADDLoss.forward (add_loss.py:101-150).
 *
 * Meshes are packed: points[3*(off[o] + k) + {0,1,2}] for object slot o,
 * npts[o] == 0 marks an absent object (the reference skips such samples,
 * add_loss.py:171-172); obj_ids outside [0, n_slots) are absent too.
 * sym[o] != 0 for SYMMETRIC_OBJECT_IDS (add_loss.py:10); diam[o] in metres.
 * Per sample b the kernels write
 *   add[b]   = mean_k ||Q_k - G_k||                         (add_loss.py:182)
 *   adds[b]  = mean_k min_j ||Q_k - G_j||                    (add_loss.py:186-189)
 *   valid[b] = 1 if the object is known, else 0
 *   correct[b] = (sym ? adds : add) < 0.1 * diam             (add_loss.py:193-195)
 * with Q = P R_pred^T + t_pred, G = P R_gt^T + t_gt computed with torch-CPU's
 * rounding (fma order, unfused _quat_to_mat) so that the per-point minimum
 * distance and its FIRST-index argmin are bit-exact.  min_dist/argmin are
 * [B][max_npts] (argmin may be NULL); pt_add is a [B][max_npts] workspace.
 * ---------------------------------------------------------------------- */
int pose6d_add_eval(const float *pred_rot, const float *pred_trans, const float *gt_rot,
                    const float *gt_trans, const int64_t *obj_ids, int64_t B,
                    const float *points, const int32_t *off, const int32_t *npts,
                    const uint8_t *sym, const double *diam, int32_t n_slots, int32_t max_npts,
                    float *min_dist, int32_t *argmin, float *pt_add,
                    double *add, double *adds, int32_t *valid, int32_t *correct, void *stream);

/* pose6d_add_eval with a neighbour table (round 6): nbr [total points][K] uint16
 * (K = 8, 16 or 32; 16-byte aligned; <= 65536 points per mesh) lists, for every mesh
 * point, other points of the same mesh near it in model space (pose6d_add_neighbors).
 * The ADD-S search first visits each point's own ground-truth point and those
 * neighbours, so the full sweep seldom finds a better candidate; its first-index tie
 * rule does not depend on the visiting order, so the results are identical (bit for
 * bit) to pose6d_add_eval whatever the table holds.  nbr == NULL: pose6d_add_eval. */
int pose6d_add_eval_nbr(const float *pred_rot, const float *pred_trans, const float *gt_rot,
                        const float *gt_trans, const int64_t *obj_ids, int64_t B,
                        const float *points, const int32_t *off, const int32_t *npts,
                        const uint8_t *sym, const double *diam, int32_t n_slots, int32_t max_npts,
                        const uint16_t *nbr, int32_t K, float *min_dist, int32_t *argmin, float *pt_add,
                        double *add, double *adds, int32_t *valid, int32_t *correct, void *stream);

/* The neighbour table of a packed mesh table (points / off / npts as pose6d_add_eval):
 * nbr[off[o] + k][0..K) = the K nearest other points of mesh o to its point k (local
 * indices; fp32 model-space distances; a mesh of fewer than K + 1 points repeats k).
 * One launch, a setup step per table (not per evaluation). */
int pose6d_add_neighbors(const float *points, const int32_t *off, const int32_t *npts, int32_t n_slots,
                         int32_t max_npts, int32_t K, uint16_t *nbr, void *stream);

/* The validation pass's epoch table (the per-batch eval_metrics of the reference's
 * training scripts, train_rgbd_geometric.py:119-146, kept on the device until the epoch
 * ends): appends one batch's per-sample results at a device-resident cursor, so a
 * replayed graph appends without the host knowing the row.
 * add/adds/valid/correct [B]: the outputs of a pose6d_add_eval[_nbr] call.
 * table [capacity][4] doubles, one row per sample: (add, adds, valid, correct).
 * state int64[2] = {rows used, batches refused}.
 * Writes rows state[0] .. state[0]+B-1, then state[0] += B.
 * If state[0] + B > capacity: writes no row, leaves state[0], state[1] += 1.
 * One workgroup; ordered against the calls before and after it by the stream alone.
 * 0 <= B <= 65535, capacity >= 0; B == 0 touches nothing.  The values are stored exactly. */
int pose6d_val_append(const double *add, const double *adds, const int32_t *valid,
                      const int32_t *correct, int64_t B, double *table,
                      int64_t capacity, int64_t *state, void *stream);

/* Backward of ADDLoss.forward (add_loss.py:101-150) w.r.t. the predicted pose:
 * loss = mean over known samples of mean_k ||Q_k - G*_k|| (G* = G_k, or the
 * nearest ground-truth point for SYMMETRIC_OBJECT_IDS, taken from the `argmin`
 * [B][max_npts] a pose6d_add_eval call on the same inputs produced); dloss is a
 * device scalar.  grad_rot [B][4] (through _quat_to_mat, add_loss.py:203-215),
 * grad_trans [B][3]; unknown objects get zero gradient. */
int pose6d_add_loss_bwd(const float *pred_rot, const float *pred_trans, const float *gt_rot,
                        const float *gt_trans, const int64_t *obj_ids, int64_t B, const float *points,
                        const int32_t *off, const int32_t *npts, const uint8_t *sym, int32_t n_slots,
                        int32_t max_npts, const int32_t *argmin, const float *dloss, float *grad_rot,
                        float *grad_trans, void *stream);

/* ADDLoss.forward / train_loss (add_loss.py:101-154) as a term of the whole-step trainers'
 * criterion: runs right after the step's head + PoseLoss launch (pose6d_geo_head_loss,
 * pose6d_quat_head_loss, pose6d_zgeo_head_loss) on the same raw / trans and ADDS
 * add_weight * L and its gradient to what that launch wrote.  No host synchronisation, no
 * allocation, everything (obj_ids included) read from device memory at run time, so a
 * replayed graph follows new obj_ids.  Two launches: one workgroup per sample, then one
 * workgroup that sums the samples in a fixed order (bitwise repeatable).
 *   raw [B][4]: the head's unnormalised quaternion; q = normalize(raw) with norm_mode as
 *     pose6d_rownorm_* (0: F.normalize, 1: x / (||x|| + 1e-8)).
 *   trans [B][3]: the step's translation (whatever trans_mode says).
 *   obj_ids int64 [B]; points / off / npts / sym / n_slots / max_npts: the packed mesh
 *     table of pose6d_add_eval.  nbr / K: the optional neighbour table of
 *     pose6d_add_eval_nbr (NULL: none); it only shortens the ADD-S search, the index found
 *     does not depend on it.
 *   per sample b: Q = P R(q)^T + trans, G = P R(gt_rot)^T + gt_trans (torch-CPU's rounding,
 *     as pose6d_add_eval); G*_k = G_k, or for a symmetric object the nearest G_j (first
 *     index on ties, searched only for symmetric samples); per[b] = mean_k ||Q_k - G*_k||.
 *   L = (1 / count) sum of per[b] over the samples whose object is known and has points
 *     (count of them); count == 0: L = 0 and nothing is added anywhere.
 * Accumulated:
 *   loss[0]     += add_weight * L
 *   grad_raw[b] += add_weight * dL/draw[b]  (through _quat_to_mat, add_loss.py:203-215, and the
 *                  normalise; a zero distance contributes zero, as torch's norm backward)
 *   trans_mode 0 (a learned translation head): grad_trans [B][3] += add_weight * dL/dtrans
 *   trans_mode 1 (a translation that is not learned): grad_trans is not touched (may be NULL)
 *   trans_mode 2 (pinhole of a learned depth z): grad_trans is grad_z [B];
 *     grad_z[b] += add_weight * (dL/dt0 (u - cx) / fx + dL/dt1 (v - cy) / fy + dL/dt2)
 *     (pose6d_pinhole_z_bwd's formula; needs bbox_center [B][2] and cam_K [B][3][3]
 *     (K_batched = 1) or [3][3] (0); both are ignored in the other modes)
 * Plain writes: per [B] doubles (0 for an unknown sample) and, if not NULL, nearest
 * [B][max_npts] int32, the ground-truth index used per point (k itself for an asymmetric
 * sample; rows of unknown samples and columns >= npts are not written).
 * 0 < B <= 65535, norm_mode 0 / 1, trans_mode 0 / 1 / 2. */
int pose6d_add_head_loss(const float *raw, int32_t norm_mode, const float *trans, const float *gt_rot,
                         const float *gt_trans, const int64_t *obj_ids, int64_t B, const float *points,
                         const int32_t *off, const int32_t *npts, const uint8_t *sym, int32_t n_slots,
                         int32_t max_npts, const uint16_t *nbr, int32_t K, float add_weight,
                         int32_t trans_mode, const float *bbox_center, const float *cam_K,
                         int32_t K_batched, float *loss, float *grad_raw, float *grad_trans, double *per,
                         int32_t *nearest, void *stream);

/* ------------------------------------------------------------------------
 * Pose heads and loss
 * ---------------------------------------------------------------------- */
/* F.normalize(x, p=2, dim=1) (mode 0: x / max(||x||, 1e-12), pose_net_rgb.py:61,
 * pose_net_rgbd.py:138, pose_net_rgbd_geometric.py:45) or the RGB-Geometric form
 * x / (||x|| + 1e-8) (mode 1, pose_net_rgb_geometric.py:75).  x, y: [B][D]. */
int pose6d_rownorm_fwd(const float *x, float *y, int64_t B, int32_t D, int32_t mode, void *stream);
int pose6d_rownorm_bwd(const float *x, const float *dy, float *dx, int64_t B, int32_t D, int32_t mode,
                       void *stream);

/* PoseNetRGBDGeometric._compute_pinhole_translation (pose_net_rgbd_geometric.py:56-85):
 * depth_raw [B][H][W] fp32 (sampled at the clamped int pixel, 223 hard-coded as in
 * the reference), bbox_center [B][2], K [B][3][3] (K_batched=1) or [3][3] (0) -> t [B][3]. */
int pose6d_pinhole_depth(const float *depth_raw, int32_t H, int32_t W, const float *bbox_center,
                         const float *K, int32_t K_batched, int64_t B, float *t, void *stream);

/* PoseNetRGBGeometric._compute_pinhole_translation (pose_net_rgb_geometric.py:93-109):
 * z [B] -> t [B][3]; backward gives dz from dt. */
int pose6d_pinhole_z_fwd(const float *z, const float *bbox_center, const float *K, int32_t K_batched,
                         int64_t B, float *t, void *stream);
int pose6d_pinhole_z_bwd(const float *dt, const float *bbox_center, const float *K, int32_t K_batched,
                         int64_t B, float *dz, void *stream);

/* PoseLoss.forward (pose_loss.py:19-28): rot_mode 0 = geodesic (:30-50),
 * 1 = quaternion L1 (:52-61); trans = l1_loss mean.  loss: one float.
 * Backward: dloss (device scalar) -> grad_rot [B][4], grad_trans [B][3]. */
int pose6d_pose_loss_fwd(const float *pred_rot, const float *pred_trans, const float *gt_rot,
                         const float *gt_trans, int64_t B, float rot_weight, float trans_weight,
                         int32_t rot_mode, float *loss, void *stream);
int pose6d_pose_loss_bwd(const float *pred_rot, const float *pred_trans, const float *gt_rot,
                         const float *gt_trans, int64_t B, float rot_weight, float trans_weight,
                         int32_t rot_mode, const float *dloss, float *grad_rot, float *grad_trans,
                         void *stream);

/* The RGBD-Geometric training step's head + loss in one launch: rot =
 * F.normalize(raw) (pose_net_rgbd_geometric.py:45), trans = pinhole(depth_raw)
 * (:56-85), loss = PoseLoss(rot, trans) (pose_loss.py:19-28) and its gradient for
 * dloss = 1: grad_raw (through the normalize) and grad_trans.  Same formulas as the
 * separate pose6d_rownorm_* / pinhole_depth / pose_loss_* calls. */
int pose6d_geo_head_loss(const float *raw, const float *depth_raw, int32_t H, int32_t W, const float *bbox_center,
                         const float *K, int32_t K_batched, const float *gt_rot, const float *gt_trans, int64_t B,
                         float rot_weight, float trans_weight, int32_t rot_mode, float *rot, float *trans,
                         float *loss, float *grad_raw, float *grad_trans, void *stream);

/* PoseNetRGB's training-step head + loss in one launch (pose6d_geo_head_loss without the
 * pinhole): rot = normalize(raw) with norm_mode as pose6d_rownorm_* (0: F.normalize,
 * pose_net_rgb.py:61; 1: x / (||x|| + 1e-8)), trans [B][3] is the translation head's
 * output as it is, loss = PoseLoss(rot, trans) (pose_loss.py:19-28) and its gradient for
 * dloss = 1: grad_raw [B][4] (through the normalise) and grad_trans [B][3].  rot, loss and
 * grad_trans are bit-identical to pose6d_rownorm_fwd + pose6d_pose_loss_fwd / _bwd. */
int pose6d_quat_head_loss(const float *raw, const float *trans, const float *gt_rot, const float *gt_trans, int64_t B,
                          float rot_weight, float trans_weight, int32_t rot_mode, int32_t norm_mode, float *rot,
                          float *loss, float *grad_raw, float *grad_trans, void *stream);

/* PoseNetRGBGeometric's training-step head + loss in one launch: rot = raw / (||raw|| + 1e-8)
 * (pose6d_rownorm_* mode 1, pose_net_rgb_geometric.py:75), trans = ((u - cx) z / fx,
 * (v - cy) z / fy, z) from the predicted depth z [B] (no clamps: pose6d_pinhole_z_fwd's
 * arithmetic, pose_net_rgb_geometric.py:93-109), loss = PoseLoss(rot, trans)
 * (pose_loss.py:19-28) and its gradient for dloss = 1: grad_raw [B][4] (through the
 * normalise) and grad_z [B] (sign(trans - gt) * trans_weight / (3 B) folded through the
 * pinhole: pose6d_pinhole_z_bwd's formula).  rot, trans and loss are bit-identical to
 * pose6d_rownorm_fwd + pose6d_pinhole_z_fwd + pose6d_pose_loss_fwd.  B > 0, rot_mode 0 / 1. */
int pose6d_zgeo_head_loss(const float *raw, const float *z, const float *bbox_center, const float *K,
                          int32_t K_batched, const float *gt_rot, const float *gt_trans, int64_t B,
                          float rot_weight, float trans_weight, int32_t rot_mode, float *rot, float *trans,
                          float *loss, float *grad_raw, float *grad_z, void *stream);

/* ------------------------------------------------------------------------
 * Input crops -- replaces the per-sample body of LineMODDatasetRGBD.__getitem__
 * after the file reads (data/dataset_rgbd.py:104-206; dataset_rgb.py:95-145 for
 * the RGB models): square crop x1.2 around the (jittered) bbox with zero padding,
 * cv2.resize(..., (S, S)) INTER_LINEAR, ToTensor + Normalize, depth / 1000 and
 * the (d - 0.1) / 1.5 normalisation, crop-adjusted centre and intrinsics.
 * rgb [B][H][W][3] uint8 (RGB; bgr != 0: cv2.imread's BGR order, the
 * cvtColor of dataset_rgbd.py:90 folded in); depth [B][H][W] uint16 mm or NULL
 * (= zeros, :94-95); bbox_orig / bbox_aug [B][4] int32 (x, y, w, h) before /
 * after the jitter of :110-118 (drawn on the host, np.random order); K [B][3][3].
 * mean_std: 6 device floats (mean[3], std[3]) or NULL (ToTensor only).
 * Outputs (each may be NULL): rgb_out [B][3][S][S], depth_out [B][1][S][S],
 * depth_raw_out [B][S][S], center_out [B][2], K_out [B][3][3], all fp32.
 * ---------------------------------------------------------------------- */
int pose6d_crop_rgbd(const uint8_t *rgb, int32_t bgr, const uint16_t *depth, int32_t B, int32_t H, int32_t W,
                     const int32_t *bbox_orig, const int32_t *bbox_aug, const float *K, int32_t S,
                     const float *mean_std, float *rgb_out, float *depth_out, float *depth_raw_out,
                     float *center_out, float *K_out, void *stream);

/* ----------------------------------------------------------------------
 * Train transform of the same crops (train_rgbd_geometric.py:41-47, applied by
 * dataset_rgbd.py:196-197): pose6d_crop_rgbd's crop + resize, then on the uint8
 * crop ColorJitter(brightness, contrast, saturation, hue) with torchvision's op
 * order / factor draws and Pillow's arithmetic, ToTensor + Normalize, then
 * RandomErasing(erase_p, (erase_scale_lo, _hi), (erase_ratio_lo, _hi), value 0).
 * A jitter value of 0 switches that op off (torchvision's None).  Random draws:
 * counter-based (seed, crop, draw) -- the same seed gives the same crops; each crop's
 * drawn parameters go to params_out [B][16] (may be NULL): perm[4], brightness,
 * contrast, saturation, hue factor (NaN = off), erase i, j, h, w (-1 = none), 0 x 4.
 * workspace: pose6d_crop_train_workspace(B, S) bytes (the uint8 crops).  S <= 232.
 * rgb_out is required; the depth / centre / K outputs as pose6d_crop_rgbd.
 * ---------------------------------------------------------------------- */
int64_t pose6d_crop_train_workspace(int32_t B, int32_t S);
int pose6d_crop_rgbd_train(const uint8_t *rgb, int32_t bgr, const uint16_t *depth, int32_t B, int32_t H, int32_t W,
                           const int32_t *bbox_orig, const int32_t *bbox_aug, const float *K, int32_t S,
                           const float *mean_std, float brightness, float contrast, float saturation, float hue,
                           float erase_p, float erase_scale_lo, float erase_scale_hi, float erase_ratio_lo,
                           float erase_ratio_hi, uint64_t seed, uint8_t *workspace, float *rgb_out, float *depth_out,
                           float *depth_raw_out, float *center_out, float *K_out, float *params_out, void *stream);

/* ----------------------------------------------------------------------
 * The same crops drawn by index from a device-resident frame store: one launch turns
 * B sample indices into the B model inputs AND labels of the reference's collated
 * batch (dataset_rgbd.py:206 / dataset_rgb.py:147).  The per-pixel arithmetic is
 * pose6d_crop_rgbd's own body.
 * Store: rgb_store [n_frames][H][W][3] uint8, depth_store [n_frames][H][W] uint16 or
 * NULL (= zeros); all offsets into it are 64-bit.  Per-sample tables, n_samples rows,
 * device: frame_of int32 (the sample's frame), bbox [.][4] int32 (x, y, w, h, before
 * the jitter), K [.][9], quat [.][4], trans [.][3], obj_id int64, and center_tab
 * [.][2] or NULL.  center_tab != NULL selects the RGB datasets' outputs: center_out and
 * K_out are plain gathers of center_tab and K (the original-image centre and
 * intrinsics, dataset_rgb.py:96,139-141); NULL: the crop-adjusted values of
 * pose6d_crop_rgbd, from the table's bbox and K.
 * Batch: sample_idx [B] int64, DEVICE memory, read at kernel time (a captured launch
 * follows later writes to it); bbox_aug [B][4] int32 device (the jittered boxes, row
 * b for crop b) or NULL (= the table's bbox).  B <= 65535.
 * Outputs (each may be NULL): those of pose6d_crop_rgbd plus quat_out [B][4],
 * trans_out [B][3], obj_out [B] int64, copied exactly from the tables.
 * Bad indices cannot fault: a sample_idx[b] outside [0, n_samples) reads nothing from
 * the tables or the store, a frame_of value outside [0, n_frames) nothing from the
 * store; that crop's outputs are zeros, obj_out[b] = -1, and *status (one device
 * int32, may be NULL; the caller zeroes it) is raised to b + 1 by atomicMax -- zero
 * after any number of launches means every index was good.  B == 0 launches nothing.
 * ---------------------------------------------------------------------- */
int pose6d_crop_rgbd_indexed(const uint8_t *rgb_store, int32_t bgr, const uint16_t *depth_store, int64_t n_frames,
                             int32_t H, int32_t W, const int32_t *frame_of, const int32_t *bbox, const float *K,
                             const float *center_tab, const float *quat, const float *trans, const int64_t *obj_id,
                             int64_t n_samples, const int64_t *sample_idx, const int32_t *bbox_aug, int32_t B,
                             int32_t S, const float *mean_std, float *rgb_out, float *depth_out,
                             float *depth_raw_out, float *center_out, float *K_out, float *quat_out,
                             float *trans_out, int64_t *obj_out, int32_t *status, void *stream);

/* pose6d_crop_rgbd_train on the indexed crops: the indexed crop into the uint8
 * workspace (pose6d_crop_train_workspace(B, S) bytes), then the train transform,
 * unchanged -- the same seed on the same resolved frames and boxes gives
 * pose6d_crop_rgbd_train's bits and params_out.  rgb_out is required, S <= 232.  A
 * crop with a bad index is transformed from an all-zero uint8 crop (its rgb_out is
 * defined but not zero); its other outputs and *status are as above. */
int pose6d_crop_rgbd_train_indexed(const uint8_t *rgb_store, int32_t bgr, const uint16_t *depth_store,
                                   int64_t n_frames, int32_t H, int32_t W, const int32_t *frame_of,
                                   const int32_t *bbox, const float *K, const float *center_tab, const float *quat,
                                   const float *trans, const int64_t *obj_id, int64_t n_samples,
                                   const int64_t *sample_idx, const int32_t *bbox_aug, int32_t B, int32_t S,
                                   const float *mean_std, float brightness, float contrast, float saturation,
                                   float hue, float erase_p, float erase_scale_lo, float erase_scale_hi,
                                   float erase_ratio_lo, float erase_ratio_hi, uint64_t seed, uint8_t *workspace,
                                   float *rgb_out, float *depth_out, float *depth_raw_out, float *center_out,
                                   float *K_out, float *quat_out, float *trans_out, int64_t *obj_out,
                                   float *params_out, int32_t *status, void *stream);

/* pose6d_crop_rgbd_train_indexed with the seed in DEVICE memory: `seed` points at one
 * uint64, read at kernel time and uniform over the launch, so the call can be captured
 * into a graph and every replay follows later writes to the word.  Everything else --
 * the device code, the outputs, params_out -- is pose6d_crop_rgbd_train_indexed's: the
 * same seed value gives the same bits. */
int pose6d_crop_rgbd_train_indexed_dseed(const uint8_t *rgb_store, int32_t bgr, const uint16_t *depth_store,
                                         int64_t n_frames, int32_t H, int32_t W, const int32_t *frame_of,
                                         const int32_t *bbox, const float *K, const float *center_tab,
                                         const float *quat, const float *trans, const int64_t *obj_id,
                                         int64_t n_samples, const int64_t *sample_idx, const int32_t *bbox_aug,
                                         int32_t B, int32_t S, const float *mean_std, float brightness,
                                         float contrast, float saturation, float hue, float erase_p,
                                         float erase_scale_lo, float erase_scale_hi, float erase_ratio_lo,
                                         float erase_ratio_hi, const uint64_t *seed, uint8_t *workspace,
                                         float *rgb_out, float *depth_out, float *depth_raw_out, float *center_out,
                                         float *K_out, float *quat_out, float *trans_out, int64_t *obj_out,
                                         float *params_out, int32_t *status, void *stream);

/* ----------------------------------------------------------------------
 * The training epoch on the device (the loop of the reference's training scripts,
 * train_rgbd_geometric.py:92-115): the host plans the epoch once -- which samples, which
 * jittered boxes, which transform seed each step takes -- and uploads it; a replayed graph
 * then takes row after row at a device-resident cursor and keeps its loss on the device.
 * Both entry points run ONE workgroup and are ordered against the calls before and after
 * them by the stream alone, like pose6d_val_append.
 *
 * pose6d_plan_next: idx_plan [steps][B] int64, bbox_plan [steps][B][4] int32 or NULL,
 * seed_plan [steps] uint64 or NULL; state int64[2] = {cursor, steps refused}.
 * cursor < steps: row `cursor` is copied to sample_idx [B], bbox_aug [B][4] (required
 * exactly when bbox_plan is given) and seed_out [1] (required exactly when seed_plan is
 * given), then cursor += 1.  cursor >= steps (or negative): no output is written and
 * state[1] += 1.  0 <= B <= 65535, steps >= 0; B == 0 touches nothing. */
int pose6d_plan_next(const int64_t *idx_plan, const int32_t *bbox_plan, const uint64_t *seed_plan, int64_t steps,
                     int64_t B, int64_t *state, int64_t *sample_idx, int32_t *bbox_aug, uint64_t *seed_out,
                     void *stream);

/* pose6d_loss_append: the step's loss (one device fp32) becomes table[rows]; state
 * int64[3] = {rows, appends refused, non-finite values stored}.  The value's 32 bits are
 * stored unchanged (NaN payloads, -0.0); a NaN or an infinity also counts in state[2].
 * rows >= capacity: nothing is written and state[1] += 1.  capacity >= 0. */
int pose6d_loss_append(const float *loss, float *table, int64_t capacity, int64_t *state, void *stream);

/* ----------------------------------------------------------------------
 * Detection crops -- the per-detection body of the reference's inference scripts up
 * to the model call (scripts/inference/inference_rgbd_geometric.py:110-182; the other
 * three scripts use subsets of it): one launch turns N detector boxes over F frames
 * into the model inputs.
 * frames [F][H][W][3] uint8 (bgr as pose6d_crop_rgbd), depth [F][H][W] uint16 mm or
 * NULL (= zeros); frame_of [N] int32 device or NULL (every detection on frame 0);
 * boxes_xyxy [N][4] int32 (x1, y1, x2, y2) DEVICE memory read at kernel time (a
 * captured launch follows later writes); K DOUBLE, [9] or, with K_per_frame != 0,
 * [F][9] (the reference's DEFAULT_K is float64 and the scripts' arithmetic on it runs
 * in Python double).  N <= 65535.
 * Geometry (:118-135): pose6d_crop_rgbd's square crop on (x1, y1, x2 - x1, y2 - y1).
 * RGB: pose6d_crop_rgbd's 8U resize, ToTensor, Normalize, unchanged.  Depth: resized
 * as FLOAT32 (:142: cv2.resize(crop_depth.astype(np.float32))): the 16U path's
 * coefficients and mul + add without its rounding to whole millimetres and saturation
 * (exact 2x: (a + b + c + d) * 0.25f), then / 1000.f and the same normalisation on
 * the unrounded value -- depth outputs differ from pose6d_crop_rgbd's by up to half a
 * millimetre.
 * Outputs (each may be NULL), fp32: rgb_out [N][3][S][S], depth_out [N][1][S][S],
 * depth_raw_out [N][S][S];
 * center_crop_out [N][2] = f32((c_box + pad - (crop origin + pad)) * scale) clipped
 * to [0, S - 1], scale = S / crop side, all in double before the one cast (:145-153);
 * K_crop_out [N][9] (:156-167), double then one cast: k_mode 0 = the script's
 * cx_crop = (cx + pad_l - crop_x1) * scale with the UNPADDED origin crop_x1; k_mode 1
 * = the dataset's (cx - crop_x1) * scale (dataset_rgbd.py:159-169, where the origin
 * has the pad added back).  The script's value is pad_l * scale (pad_t * scale)
 * larger on a box padded at the left (top); the models were trained on the
 * dataset's;
 * center_img_out [N][2] = f32 of the box centre, K_img_out [N][9] = f32(K)
 * (inference_rgb_geometric.py:105-106).
 * A frame_of[b] outside [0, F) reads nothing: detection b's outputs are zeros and
 * *status (one device int32, may be NULL; the caller zeroes it) is raised to b + 1 by
 * atomicMax.  N == 0 launches nothing.
 * ---------------------------------------------------------------------- */
int pose6d_crop_detections(const uint8_t *frames, int32_t bgr, const uint16_t *depth, int32_t F, int32_t H, int32_t W,
                           const int32_t *frame_of, const int32_t *boxes_xyxy, int32_t N, const double *K,
                           int32_t K_per_frame, int32_t S, const float *mean_std, int32_t k_mode, float *rgb_out,
                           float *depth_out, float *depth_raw_out, float *center_crop_out, float *K_crop_out,
                           float *center_img_out, float *K_img_out, int32_t *status, void *stream);

/* ----------------------------------------------------------------------
 * What the inference scripts do after the model call, for N detections in one launch,
 * in fp64 as the reference's host numpy: translation correction, then the projection
 * of 12 points per detection -- the object's 8 box corners, the origin and the three
 * axis tips at axis_scale (utils/visualization.py:8-32, :63-66).
 * quat [N][4] fp32 (x, y, z, w: scipy's order), trans [N][3] fp32; K double [9] or
 * [F][9] with frame_of [N] (K_per_frame as above; F >= 1); obj [N] int64 rows into
 * corners [n_obj][8][3] double.
 * Translation: boxes_xyxy != NULL (the RGB and RGBD scripts, inference_rgb.py:99-104):
 * z = (double)trans[2], x = (c_x_box - cx) * z / fx, y alike; NULL: (double)trans.
 * Rotation: scipy's Rotation.from_quat(q).as_matrix() -- cast to double, divide by the
 * norm, the unit-quaternion matrix (csrc/pose_geom.h's quat_load / quat_unit / quat_to_mat,
 * which the two depth stages below share; the sign quat_unit may flip cancels in every entry
 * of the matrix).  Projection: p = R c + t, z = max(p.z, 0.001),
 * u = p.x * K00 / z + K02, v alike.
 * Outputs (each may be NULL): trans_out [N][3] double, pts_out [N][12][2] double,
 * pix_out [N][12][2] int64 = the points truncated toward zero (numpy's astype(int));
 * a NaN, an infinity or a value outside int64 gives INT64_MIN, as numpy does on
 * x86-64.  valid_out [N] uint8: 0, with that detection's rows zeroed, for an obj
 * outside [0, n_obj) (the scripts skip an object without a mesh), a quaternion whose
 * norm is zero or NaN (scipy raises on zero) or a frame_of outside [0, F).
 * ---------------------------------------------------------------------- */
int pose6d_pose_project(const float *quat, const float *trans, const int32_t *boxes_xyxy, const double *K,
                        int32_t K_per_frame, const int32_t *frame_of, int32_t F, const int64_t *obj,
                        const double *corners, int64_t n_obj, double axis_scale, int32_t N, double *trans_out,
                        double *pts_out, int64_t *pix_out, uint8_t *valid_out, void *stream);

/* ----------------------------------------------------------------------
 * Depth refinement: point-to-point ICP of N estimated poses against the depth frame
 * their detections were cropped from, ONE launch, one workgroup per detection.  The
 * reference project has no such step; the arithmetic contract below is restated in
 * fp64 numpy by tests/refine_ref.py.
 * depth [F][H][W] uint16 raw units, metres = d * depth_scale; K double [9] or [F][9]
 * with frame_of (K_per_frame as pose6d_pose_project); boxes_xyxy [N][4] int32; frame_of
 * [N] int32 or NULL (frame 0); obj [N] int64 slots of the packed mesh table points /
 * off / npts / diam / n_slots of pose6d_add_eval; quat [N][4] fp32 (x, y, z, w), model
 * -> camera, normalised in double here; trans [N][3] double.
 * Samples: G x G per box, sample k = j * G + i at pixel u = x1 + floor((2i + 1)(x2 -
 * x1) / (2G)), v alike from j, y1, y2 (integers): csrc/pose_geom.h's sample_pixel, which
 * pose6d_pose_verify calls too.  Valid inside the frame with depth > 0 (its depth_at: 0
 * outside the frame); back-projected in double, z = d * depth_scale, x = (u - cx) * z / fx, y alike,
 * every product rounded on its own; kept when sqrt(|p - trans|^2) <= gate * diam -- the
 * gate centre is the INITIAL translation in every iteration.
 * `iters` times: q = R^T (p - t) in double, rounded to fp32; the nearest mesh point by
 * direct fp32 differences s = fma(dz, dz, fma(dy, dy, dx * dx)), first index on a tie;
 * accepted when sqrt((double)s) <= trim * diam; over the accepted pairs n, sum p, sum m,
 * sum m p^T in double (p relative to the initial translation) in a fixed order; n <
 * min_points stops and keeps the last pose; else Horn's closed form (cyclic Jacobi on
 * the 4 x 4 symmetric matrix, a fixed number of sweeps) gives a unit quaternion, w >=
 * 0, hence a proper rotation, and t = mean p - R mean m.
 * Outputs: quat_out [N][4] double (unit, w >= 0), trans_out [N][3] double, quat32_out /
 * trans32_out their float casts (may be NULL), n_corr [N] int32 (accepted pairs of the
 * last completed iteration), rms [N][2] double (root mean square accepted distance of
 * the first and the last completed iteration), refined [N] uint8.  refined = 0 with the
 * input pose passed through (the quaternion normalised where it can be) and zeros
 * elsewhere: obj outside the table or without points, a zero / NaN quaternion, frame_of
 * outside [0, F), fewer than min_points accepted pairs in the first iteration.
 * Debug outputs, NULL in the product path: pose_trace [N][iters + 1][7] double (x, y,
 * z, w, tx, ty, tz before iteration 0 and after each; the last pose repeats after a
 * stop), corr_out [N][iters][P] int32 (the accepted mesh index; -1 invalid, gated out
 * or trimmed; -2 iteration not completed), samples_out [N][P][3] double (the kept
 * samples' camera points, NaN for the others).
 * G in [1, 32], iters in [1, 64], min_points >= 3, gate, trim, depth_scale > 0.
 * ---------------------------------------------------------------------- */
int pose6d_depth_refine(const uint16_t *depth, int32_t F, int32_t H, int32_t W, double depth_scale, const double *K,
                        int32_t K_per_frame, const int32_t *boxes_xyxy, const int32_t *frame_of, const int64_t *obj,
                        const float *points, const int32_t *off, const int32_t *npts, const double *diam,
                        int32_t n_slots, const float *quat, const double *trans, int32_t N, int32_t G, int32_t iters,
                        double gate, double trim, int32_t min_points, double *quat_out, double *trans_out,
                        float *quat32_out, float *trans32_out, int32_t *n_corr, double *rms, uint8_t *refined,
                        double *pose_trace, int32_t *corr_out, double *samples_out, void *stream);

/* ----------------------------------------------------------------------
 * Pose verification: render-and-compare of N poses against the depth frame, ONE launch,
 * one workgroup per detection.  The object's triangle mesh is rendered at the pose into a
 * G x G z-buffer over the detection box and every sample is compared with the observed
 * depth.  The reference project has no such step; the arithmetic contract below is
 * restated in fp64 numpy by tests/verify_ref.py.  Everything is double, every product
 * rounded on its own.
 * depth, depth_scale, K, K_per_frame, boxes_xyxy, frame_of, F, obj: as
 * pose6d_depth_refine; obj [N] int64 are slots of the packed TRIANGLE table: verts float
 * [sum V][3] metres, faces int32 [sum T][3] (indices local to the object), voff / nverts /
 * toff / ntri int32 [n_slots] (first vertex, vertex count, first triangle, triangle
 * count), diam double [n_slots].  quat [N][4] fp32 (x, y, z, w), normalised in double by
 * the code pose6d_depth_refine runs (csrc/pose_geom.h's read_detection: one header reader
 * for both entry points); trans [N][3] double.
 * Vertices: c = R m + t, each row summed left to right; pu = c.x * fx / c.z + cx, pv
 * alike.  A triangle is skipped when an index is outside [0, nverts) (never
 * dereferenced), a vertex has c.z <= 0.001 or a projected coordinate is not finite.
 * Samples: pose6d_depth_refine's G x G grid (the same sample_pixel), sample k = j * G + i
 * at the integer pixel p.
 * Coverage: e(a, b, p) = (b.u - a.u)(p.v - a.v) - (b.v - a.v)(p.u - a.u); w0 = e(v1, v2,
 * p), w1 = e(v2, v0, p), w2 = e(v0, v1, p), s = (w0 + w1) + w2; covered when all three w
 * >= 0 and s > 0, or all three <= 0 and s < 0 (both windings, inclusive edges, no
 * back-face culling), and p lies inside the triangle's pixel bounding box -- implied in
 * exact arithmetic, stated so that culling by the box is exact in floating point.  The
 * rendered depth is z = s / ((w0 / z0 + w1 / z1) + w2 / z2), kept when positive and
 * finite; the z-buffer holds the minimum per sample.  The result is DEFINED by every
 * triangle against every sample; the kernel only skips what the box test excludes.
 * Classes, from d = depth[v][u] (0 outside the frame) and z_obs = d * depth_scale: 0 no
 * hit; 1 hit, d == 0; 2 consistent, |z_obs - z| <= tau * diam; 3 occluded, z_obs - z <
 * -tau * diam; 4 violated, z_obs - z > tau * diam.
 * Outputs: counts [N][5] int32; fit [N] double = n2 / (n2 + n3 + n4); agree [N] double =
 * n2 / (n2 + n4) (both 0 on a zero denominator); resid [N] double, the mean |z_obs - z|
 * over class 2 (0 without one), summed in a fixed order; verified [N] uint8.  verified =
 * 0 with zeros elsewhere: obj outside the table or a slot without triangles, a zero / NaN
 * / infinite quaternion, frame_of outside [0, F).
 * Optional, NULL in the product path: zbuf_out [N][P] double (+inf: no hit) and cls_out
 * [N][P] uint8 (P = G * G); a detection with verified = 0 has +inf and 0 there.
 * Optional choice between two poses of the same detections (best needs both others):
 * best [N] uint8 = base_flag[n] != 0 && verified && fit >= base_fit[n], with base_fit [N]
 * double the fit of an earlier launch and base_flag [N] uint8 a condition on this pose
 * (the refiner's `refined`).
 * G in [1, 64], tau > 0 (a fraction of the diameter), depth_scale > 0, N, F, H, W >= 0.
 * ---------------------------------------------------------------------- */
int pose6d_pose_verify(const uint16_t *depth, int32_t F, int32_t H, int32_t W, double depth_scale, const double *K,
                       int32_t K_per_frame, const int32_t *boxes_xyxy, const int32_t *frame_of, const int64_t *obj,
                       const float *verts, const int32_t *faces, const int32_t *voff, const int32_t *nverts,
                       const int32_t *toff, const int32_t *ntri, const double *diam, int32_t n_slots,
                       const float *quat, const double *trans, int32_t N, int32_t G, double tau, int32_t *counts,
                       double *fit, double *agree, double *resid, uint8_t *verified, double *zbuf_out,
                       uint8_t *cls_out, const double *base_fit, const uint8_t *base_flag, uint8_t *best,
                       void *stream);

/* ------------------------------------------------------------------------
 * ResNet50 trunk — replaces torchvision.models.resnet50 children[:-1] as
 * wrapped by every model (pose_net_rgb.py:18-20, pose_net_rgb_geometric.py:18-20,
 * pose_net_rgbd.py:48-61, pose_net_rgbd_geometric.py:23-25) and the z-CNN of
 * pose_net_rgb_geometric.py:36-55.  NHWC activations of `dtype`.
 * ---------------------------------------------------------------------- */
/* model input (B, C, H, W) fp32 -> NHWC with channels zero-padded to Cpad */
int pose6d_nchw_to_nhwc(int32_t dtype, const float *x, void *y, int32_t N, int32_t C, int32_t H, int32_t W,
                        int32_t Cpad, void *stream);

/* One launch packs every conv's OIHW fp32 master weight into the kernel layouts:
 * wp [O][Kpad] (K = (kh, kw', ci): ci padded to Ip, KWp packed taps kw' per kernel
 * row with filter tap kw at kw' = kw + KWp - KW, zeros elsewhere and beyond K) and,
 * when non-null, wt [I][KH][KW][O] for the data gradient.  `descs` is a device array of
 * n_desc records of pose6d_pack_desc_size() bytes:
 *   { const float *w; void *wp; void *wt; int32 O, I, Ip, KH, KW, Kpad, KWp, reserved; int64 start; }
 * (start: the caller's bookkeeping, unused; total: sum of O*Kpad, unused).  KWp and
 * Kpad of a forward conv come from pose6d_conv_pack_geom. */
int pose6d_pack_desc_size(void);
int pose6d_pack_conv_weights(int32_t dtype, const void *descs, int32_t n_desc, int64_t total, void *stream);
/* Packed layout of a conv's forward filter (wp): taps per kernel row (*kw_packed: KW,
 * or 8 for the row-tap stems -- Cin 4, stride 2, a kernel row of <= 8 taps: 7x7 / pad 3,
 * read by the LDS-DMA kernel as 64-byte input rows) and the padded K (*Kpad). */
int pose6d_conv_pack_geom(int32_t dtype, int32_t Cin, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                          int32_t *kw_packed, int32_t *Kpad);

/* nn.Conv2d forward (implicit GEMM on MFMA).  x [N][H][W][Cin] (Cin = 4 for the
 * padded stem, else a power of two), wp packed [Cout][Kpad], y [N][Ho][Wo][Cout].
 * bias may be NULL.  stats (NULL = none) receives BatchNorm partials over blocks of
 * 32 output pixels, rows = pose6d_conv_stats_rows(...), stored channel-major
 * [2][Cout][rows] fp32: stats[c][r] = sum, stats[Cout + c][r] = M2 about the block
 * mean. */
int pose6d_conv_stats_rows(int32_t N, int32_t Ho, int32_t Wo, int32_t Cout);
int pose6d_conv2d_fwd(int32_t dtype, const void *x, const void *wp, const float *bias, void *y, float *stats,
                      int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                      int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, void *splitk_ws, int64_t splitk_ws_bytes,
                      void *stream);
/* Split-K workspace (caller-provided; the library keeps no device state of its own).
 * A forward plan on a small grid with a long K loop (pose6d_conv_variant >> 16 > 1)
 * divides each output tile's K-steps over several workgroups of one launch; their
 * fp32 partial tiles and the tiles' arrival counters live in splitk_ws:
 *   bytes = pose6d_conv_splitk_workspace(dtype, pass 0 = forward / 1 = data gradient, geometry...)
 * (0 = the plan does not split: splitk_ws may be NULL).  Layout: 32 KiB of arrival
 * counters, then the partial tiles.  The counter block must be ZERO before the first
 * use of a workspace (e.g. allocate it zeroed); every launch leaves it zero, so one
 * workspace serves any sequence of stream-ordered convs.  Launches that may run
 * concurrently (other streams, other threads) need workspaces of their own.  256-byte
 * aligned.  A plan that splits and gets no (or too small a) workspace fails with
 * POSE6D_ERR_ARG; data gradients split only under an explicit pose6d_tuning_t. */
int64_t pose6d_conv_splitk_workspace(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                     int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho,
                                     int32_t Wo);
/* kernel variant a conv launch selects (profiling joins): fwd/dgrad (pass 0/1):
 * (splits << 16) | (stages << 12) | (fast << 8) | (mode << 4) | tile (tile 0..3 = 128x128, 128x64,
 * 64x128, 64x64; mode 0 gemm, 1 im2col, 2 narrow stem, 3 dgrad, 4 stride-2 dgrad
 * split into output parity classes; fast = LDS-DMA bf16 kernel with an LDS ring
 * of `stages` K-steps, 0 on the register-staged kernel; splits = workgroups per output
 * tile of the in-launch split-K, 1 = none);
 * wgrad (pose6d_wgrad_variant, Cin = the padded channel count): (stages << 12) |
 * (fast << 8) | (BM == 128) << 1 | (BN == 128); fast = the LDS-DMA weight-gradient
 * kernel (bf16: 64x64 tiles; fp32: 64x64 or 128x128 tiles, bits 1 and 0), 0 = the
 * register-staged kernel. */
int pose6d_conv_variant(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                        int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo);
int pose6d_wgrad_variant(int32_t dtype, int32_t M, int32_t Cout, int32_t K, int32_t Cin);
/* 3x3 / stride 1 / pad 1 bf16 forwards WITHOUT BatchNorm statistics (eval: pose6d_conv2d_fwd
 * with stats == NULL, pose6d_conv2d_fwd_act) on >= 64-channel slices run the patch kernel
 * (conv3x3_patch_kernel: each workgroup stages its input patch once per 64-channel slice
 * instead of once per filter tap): its workgroup count, or 0 when the geometry takes the
 * implicit-GEMM plans pose6d_conv_variant describes. */
int pose6d_conv_patch_plan(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                           int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo);
/* eval-mode forward with the BatchNorm folded into the store: out = act(T(conv(x) [+ bias]) * scale + shift
 * [+ res | + res * res_scale + res_shift]), act = ReLU if relu -- pose6d_conv2d_fwd followed by
 * pose6d_bn_act_fwd bit for bit, one launch, no raw-output round trip.  res: NHWC like out (or NULL). */
int pose6d_conv2d_fwd_act(int32_t dtype, const void *x, const void *w, const float *bias, void *out, int32_t N,
                          int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                          int32_t pad, int32_t Ho, int32_t Wo, const float *scale, const float *shift, const void *res,
                          const float *res_scale, const float *res_shift, int32_t relu, void *splitk_ws,
                          int64_t splitk_ws_bytes, void *stream);
/* eval-mode output of a torchvision Bottleneck with a downsample branch, ONE launch
 * (replaces, at pose_net_*.py's `self.backbone(x)`, the block's conv3 + bn3 and the
 * downsample conv + bn + add + ReLU):
 *   out = act(T(x . w) * scale + shift + T(xd_s . wd) * scale_d + shift_d),
 * x [N][Ho][Wo][Cin] (conv3 input), w [Cout][Cin]; xd [N][Hd][Wd][Cind] (block input),
 * wd [Cout][Cind], xd_s = xd sampled every stride_d pixels; both 1x1, no bias.  Bit for
 * bit pose6d_conv2d_fwd of the downsample then pose6d_conv2d_fwd_act with
 * res_scale/res_shift, without the downsample output's HBM round trip.  Rejected
 * (POSE6D_ERR_ARG) when either separate launch's plan splits K (pose6d_conv_variant). */
int pose6d_conv2d_fwd_act_dual(int32_t dtype, const void *x, const void *w, const void *xd, const void *wd, void *out,
                               int32_t N, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout, int32_t Hd, int32_t Wd,
                               int32_t Cind, int32_t stride_d, const float *scale, const float *shift,
                               const float *scale_d, const float *shift_d, int32_t relu, void *stream);
/* data gradient: dx [N][H][W][Cin] = conv_transpose(dy [N][Ho][Wo][Cout], wt) (+ dres if non-NULL).
 * dres may be dx itself (accumulate in place); a stride-2 1x1 conv then writes only the
 * pixels its taps reach (the other three parity classes are left as they are). */
int pose6d_conv2d_dgrad(int32_t dtype, const void *dy, const void *wt, const void *dres, void *dx, int32_t N,
                        int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                        int32_t pad, int32_t Ho, int32_t Wo, void *stream);
/* weight gradient into OIHW fp32 dw (Cin_real channels of the Cin-padded input);
 * workspace: pose6d_conv2d_wgrad_workspace(...) bytes of fp32 split slabs, its
 * size passed as ws_bytes (a plan needing more fails with POSE6D_EINVAL). */
int64_t pose6d_conv2d_wgrad_workspace(int32_t dtype, int32_t N, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout,
                                      int32_t KH, int32_t KW);
int pose6d_conv2d_wgrad(int32_t dtype, const void *x, const void *dy, float *dw, int32_t accumulate,
                        float *workspace, int64_t ws_bytes, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cin_real,
                        int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                        void *stream);

/* Data + weight gradient of one conv in one call (pose6d_conv2d_dgrad followed by
 * pose6d_conv2d_wgrad, same arguments and workspace): on the bf16 LDS-DMA paths
 * both run as ONE launch whose workgroups split between the two passes, then
 * the slab reduce.  dx == NULL skips the data gradient. */
int pose6d_conv2d_backward(int32_t dtype, const void *x, const void *dy, const void *wt, const void *dres,
                           void *dx, float *dw, int32_t accumulate, float *workspace, int64_t ws_bytes, int32_t N,
                           int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout, int32_t KH,
                           int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, void *stream);
/* Explicit plan overrides for the conv entry points' *_tuned forms -- used by the
 * tests (every tile / ring depth / kernel of a shape must agree) and the tuning tools,
 * never by the product path: without one, each conv geometry has exactly one plan,
 * so one summation order.  Every field -1 = the default plan.
 *   conv_tile     fast path 0 = 128x128, 1 = 128x64, 3 = 64x64 (4 waves), 4 = 128x128, 5 = 128x64 (8 waves);
 *                 register-staged path 0..3 = 128x128, 128x64, 64x128, 64x64
 *   conv_stages   LDS ring slots of the fast path (2, 3, 4, 6)
 *   conv_s2       0: the stride-2 data gradient as one masked gather instead of 4 parity classes
 *   conv_base     1: the register-staged conv kernels instead of the LDS-DMA path
 *   wgrad_stages  LDS ring slots of the bf16 weight-gradient kernel (2..4)
 *   wgrad_base    1: the register-staged weight-gradient kernel (other split plan)
 *   bwd_separate  1: data and weight gradient as separate launches (not the fused kernel)
 *   conv_splitk   fast path (1x1 / KxK forward, stride-1 data gradient): K-steps of each output tile
 *                 split over this many workgroups of one launch (1 = none)
 *   wgrad_splits  weight gradient: pixel splits (slabs) of the plan (>= 1; tools only)
 *   bwd_order     fused backward: 1 = weight-gradient workgroups dispatched first, 0 = data gradient first
 *   conv_patch    3x3 stride-1 bf16 forwards without BatchNorm statistics: 0 = the implicit-GEMM plan,
 *                 1 or -1 = the patch plan (-1 only while no conv_tile / conv_stages / conv_base /
 *                 conv_splitk is forced)
 * A tuned plan that splits K needs pose6d_conv_splitk_workspace_tuned(...) bytes of
 * split-K workspace (see pose6d_conv_splitk_workspace). */
typedef struct {
  int32_t conv_tile, conv_stages, conv_s2, conv_base, wgrad_stages, wgrad_base, bwd_separate, conv_splitk;
  int32_t wgrad_splits, bwd_order, conv_patch;
} pose6d_tuning_t;
int64_t pose6d_conv_splitk_workspace_tuned(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W,
                                           int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                           int32_t pad, int32_t Ho, int32_t Wo, const pose6d_tuning_t *tuning);
int pose6d_conv2d_fwd_tuned(int32_t dtype, const void *x, const void *w, const float *bias, void *y, float *stats,
                            int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                            int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, const pose6d_tuning_t *tuning,
                            void *splitk_ws, int64_t splitk_ws_bytes, void *stream);
int pose6d_conv2d_dgrad_tuned(int32_t dtype, const void *dy, const void *wt, const void *dres, void *dx, int32_t N,
                              int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                              int32_t pad, int32_t Ho, int32_t Wo, const pose6d_tuning_t *tuning, void *splitk_ws,
                              int64_t splitk_ws_bytes, void *stream);
int64_t pose6d_conv2d_wgrad_workspace_tuned(int32_t dtype, int32_t N, int32_t Ho, int32_t Wo, int32_t Cin,
                                            int32_t Cout, int32_t KH, int32_t KW, const pose6d_tuning_t *tuning);
int pose6d_conv2d_wgrad_tuned(int32_t dtype, const void *x, const void *dy, float *dw, int32_t accumulate,
                              float *workspace, int64_t ws_bytes, int32_t N, int32_t H, int32_t W, int32_t Cin,
                              int32_t Cin_real, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                              int32_t Ho, int32_t Wo, const pose6d_tuning_t *tuning, void *stream);
int pose6d_conv2d_backward_tuned(int32_t dtype, const void *x, const void *dy, const void *wt, const void *dres,
                                 void *dx, float *dw, int32_t accumulate, float *workspace, int64_t ws_bytes,
                                 int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout,
                                 int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                 const pose6d_tuning_t *tuning, void *stream);
/* pose6d_conv2d_backward in phases (profiling): bit 0 = the gradient launch(es) that
 * fill the fp32 slabs (and dx), bit 1 = the slab reduce into dw; 3 = the whole call.
 * On the unfused path bit 0 runs the complete dgrad + wgrad and bit 1 nothing.  A
 * fused 1x1 conv whose weight gradient has ONE split and K = Cin = Cin_real, not
 * accumulating (layer4's 1x1 convs), writes dw directly during bit 0 (its single slab
 * is the OIHW gradient): bit 1 then does nothing. */
int pose6d_conv2d_backward_ex(int32_t dtype, const void *x, const void *dy, const void *wt, const void *dres,
                              void *dx, float *dw, int32_t accumulate, float *workspace, int64_t ws_bytes, int32_t N,
                              int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout, int32_t KH,
                              int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, int32_t phases,
                              void *stream);
/* Backward chaining across convs: a weight-gradient slab reduce described by
 * pose6d_wgrad_reduce_t (the conv's geometry as passed to pose6d_conv2d_backward,
 * its workspace of slabs and its dW) can ride on the NEXT conv's fused launch as
 * extra workgroups instead of a launch of its own.
 * pose6d_conv2d_backward_chain = pose6d_conv2d_backward that (a) also reduces
 * `prev` (NULL = none; its slabs must be in a different workspace) and (b) when
 * this conv runs the fused kernel, leaves its OWN reduce pending: *deferred = 1,
 * and the caller passes it as `prev` to the next call or flushes it with
 * pose6d_wgrad_reduce.  *deferred = 0: this conv's dW is complete (also the case of
 * the direct-dW plans described at pose6d_conv2d_backward_ex). */
typedef struct {
  const float *ws;
  float *dw;
  int32_t dtype, N, H, W, Cin, Cin_real, Cout, KH, KW, stride, pad, Ho, Wo, accumulate;
} pose6d_wgrad_reduce_t;
int pose6d_wgrad_reduce(const pose6d_wgrad_reduce_t *job, void *stream);
int pose6d_conv2d_backward_chain(int32_t dtype, const void *x, const void *dy, const void *wt, const void *dres,
                                 void *dx, float *dw, int32_t accumulate, float *workspace, int64_t ws_bytes,
                                 int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout,
                                 int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                 const pose6d_wgrad_reduce_t *prev, int32_t *deferred, void *stream);
/* pose6d_conv2d_backward_chain whose residual contribution is dres * mask instead of
 * dres: dres_mask = pose6d_bn_act_fwd_mask's ReLU bits for dres (bit e of byte i masks
 * element i * E + e, E = 8 bf16 / 4 fp32), i.e. dres = the block output's gradient and
 * the product = the dz a residual BN backward would otherwise write out; dres != dx. */
int pose6d_conv2d_backward_chain_masked(int32_t dtype, const void *x, const void *dy, const void *wt,
                                        const void *dres, const uint8_t *dres_mask, void *dx, float *dw,
                                        int32_t accumulate, float *workspace, int64_t ws_bytes, int32_t N, int32_t H,
                                        int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout, int32_t KH,
                                        int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                        const pose6d_wgrad_reduce_t *prev, int32_t *deferred, void *stream);

/* A BatchNorm backward's reduce pass folded into the data gradient that completes
 * its output gradient (the BN + ReLU producing this conv's input): while storing dX
 * (+ dres * mask), the epilogue also sums, per channel over each output tile,
 * dz = dX * relu and dz * (y - mean) * invstd into partial[2][C][rows] -- what
 * pose6d_bn_bwd's first launch computes from dX re-read.  relu = the stored bits
 * (relu_mask, pose6d_bn_act_fwd_mask) or T(y * relu_scale + relu_shift) > 0;
 * y2 / mean2 / invstd2 / partial2: a second BN fed the same dz (a downsampling
 * block's branch BN; needs relu_mask).  rows = pose6d_conv2d_backward_bn_rows.
 * pose6d_bn_bwd_partials then finishes the backward (finalize + apply). */
typedef struct {
  const void *y;
  const float *mean, *invstd;
  const float *relu_scale, *relu_shift;
  const uint8_t *relu_mask;
  float *partial;
  const void *y2;
  const float *mean2, *invstd2;
  float *partial2;
  int32_t rows;
} pose6d_bn_reduce_t;

int pose6d_conv2d_backward_bn_rows(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                   int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo);

/* pose6d_conv2d_backward_chain (dres_mask as in _masked, or NULL) whose data gradient
 * also produces the BatchNorm-reduce partials `bn` describes (NULL = none); dX must be
 * written whole (dres != dx). */
int pose6d_conv2d_backward_chain_bn(int32_t dtype, const void *x, const void *dy, const void *wt, const void *dres,
                                    const uint8_t *dres_mask, void *dx, float *dw, int32_t accumulate,
                                    float *workspace, int64_t ws_bytes, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                    int32_t Cin_real, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                    int32_t pad, int32_t Ho, int32_t Wo, const pose6d_wgrad_reduce_t *prev,
                                    int32_t *deferred, const pose6d_bn_reduce_t *bn, void *stream);
/* (1 << 16) | (data-gradient mode << 4) | ring stages when pose6d_conv2d_backward
 * runs ONE fused conv_bwd_kernel<mode, stages, 3> launch (+ the reduce), else 0 */
int pose6d_bwd_variant(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                       int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo);

/* nn.BatchNorm2d: finalize the conv-epilogue statistics (training) or use the
 * running statistics (eval) -> scale/shift (+ saved mean / invstd); running
 * stats, num_batches_tracked updated in training (torch semantics).
 * partial: [2][C][rows] (rows = ceil(count / 32); sum, M2 about the block's mean)
 * over 32-pixel blocks, as pose6d_conv2d_fwd writes them, folded in fp64 as shifted sums about the first row's
 * mean in ONE launch; workspace: unused (kept in the ABI, may be NULL). */
int pose6d_bn_finalize(const float *partial, int32_t rows, int32_t C, int64_t count, const float *gamma,
                       const float *beta, float *running_mean, float *running_var, int64_t *num_batches,
                       float momentum, float eps, int32_t training, float *scale, float *shift, float *save_mean,
                       float *save_invstd, double *workspace, void *stream);
/* pose6d_bn_finalize (training) of two BatchNorms over the same output grid -- a
 * downsampling Bottleneck's bn3 and its downsample BN (same rows, count) -- in ONE
 * launch; each BN's results bit for bit those of its own pose6d_bn_finalize call. */
typedef struct {
  const float *partial;   /* [2][C][rows] conv-epilogue statistics */
  const float *gamma, *beta;
  float *running_mean, *running_var;
  int64_t *num_batches;   /* may be NULL */
  float *scale, *shift, *save_mean, *save_invstd;
  float momentum, eps;
  int32_t C;
} pose6d_bn_stats_t;
int pose6d_bn_finalize_dual(const pose6d_bn_stats_t *a, const pose6d_bn_stats_t *b, int32_t rows, int64_t count,
                            void *stream);
/* Eval-mode fold of a table of BatchNorms in one launch: per entry and channel c,
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale,
 * save_mean = running_mean, save_invstd = 1 / sqrt(running_var + eps) -- pose6d_bn_finalize
 * with training = 0, for all entries.  descs: device array of n pose6d_bn_fold_t
 * (pose6d_bn_fold_desc_size() bytes each), max_c >= every entry's C. */
typedef struct {
  const float *gamma, *beta, *running_mean, *running_var;
  float *scale, *shift, *save_mean, *save_invstd;
  float eps;
  int32_t C;
} pose6d_bn_fold_t;
int pose6d_bn_fold_desc_size(void);
int pose6d_bn_eval_fold(const void *descs, int32_t n, int32_t max_c, void *stream);
/* out = act(y * scale + shift [+ res | + res * res_scale + res_shift]); act = ReLU if relu */
int pose6d_bn_act_fwd(int32_t dtype, const void *y, const float *scale, const float *shift, const void *res,
                      const float *res_scale, const float *res_shift, int32_t relu, void *out, int64_t M, int32_t C,
                      void *stream);
/* bn_act_fwd that also writes relu_mask[M * C / E] (E = 8 bf16 / 4 fp32 elements per
 * byte, bit e of byte i = out[i * E + e] > 0) for pose6d_bn_bwd_mask. */
int pose6d_bn_act_fwd_mask(int32_t dtype, const void *y, const float *scale, const float *shift, const void *res,
                           const float *res_scale, const float *res_shift, int32_t relu, void *out, uint8_t *relu_mask,
                           int64_t M, int32_t C, void *stream);
/* Training BatchNorm finalize + apply in ONE launch: pose6d_bn_finalize(bn, training = 1)
 * followed by pose6d_bn_act_fwd_mask(y, bn->scale, bn->shift, res, NULL, NULL, relu, out,
 * relu_mask), bit for bit (the identity-residual / no-residual forms; C a multiple of 64,
 * rows = ceil(count / 32) as the conv epilogue wrote them).  The apply workgroups wait for
 * the finalize workgroups of their channels through `flags` (pose6d_bn_finalize_act_flags
 * int32, zeroed ONCE by the caller, then left to the launches) and `epoch`, a device
 * int64 the caller advances (+1) between two launches on the same flags and never
 * changes while one runs; an apply workgroup that does not see its flags in time
 * computes its channels itself (same arithmetic), so nothing depends on dispatch order
 * (a NEGATIVE epoch sends every apply workgroup that way at once: tests).
 * Replaces pose6d_bn_finalize + pose6d_bn_act_fwd_mask of the trunk's training forward
 * (bn_stats_finalize / bn_act, BatchNorm2d + ReLU [+ residual] of every Bottleneck). */
int32_t pose6d_bn_finalize_act_flags(int32_t rows, int32_t C);
int pose6d_bn_finalize_act(int32_t dtype, const pose6d_bn_stats_t *bn, int32_t rows, int64_t count, const void *y,
                           const void *res, int32_t relu, void *out, uint8_t *relu_mask, int32_t *flags,
                           const int64_t *epoch, void *stream);
/* backward of bn_act_fwd for one BN: dz = dout * mask, mask = out > 0 when `out` is
 * given, else (relu_scale/relu_shift given: a ReLU BN without residual) the sign
 * bn_act_fwd stored, recomputed from y as round(y * relu_scale + relu_shift) > 0
 * (no read of the forward output), else 1; dgamma/dbeta (accumulate or
 * overwrite); dy; dz_out (if non-NULL) = dz.
 * workspace: (pose6d_bn_bwd_workspace_rows(M) * 2 + 3) * C floats. */
int pose6d_bn_bwd_workspace_rows(int64_t M);
/* pose6d_bn_bwd with the ReLU mask taken from pose6d_bn_act_fwd_mask's bits instead of
 * re-reading the forward output (the residual BNs: 1/16 of the bytes). */
int pose6d_bn_bwd_mask(int32_t dtype, const void *dout, const uint8_t *relu_mask, const void *y, const float *mean,
                       const float *invstd, const float *gamma, float *dgamma, float *dbeta, int32_t accumulate,
                       void *dy, void *dz_out, float *workspace, int64_t M, int32_t C, void *stream);
/* The rest of a BatchNorm backward whose reduce pass ran in the data gradient that
 * produced dout (pose6d_conv2d_backward_chain_bn's `partial`, [2][C][rows]): the
 * finalize (dgamma, dbeta written or accumulated) and the apply (dy), two launches.
 * relu = relu_mask bits or T(y * relu_scale + relu_shift) > 0.  partial2 / y2 / mean2 /
 * invstd2 / gamma2 / dgamma2 / dbeta2 / dy2 (or NULL partial2): a second BN fed the
 * same dout * mask (needs relu_mask).  coef: 3 * C floats (6 * C with the second BN). */
int pose6d_bn_bwd_partials(int32_t dtype, const float *partial, int32_t rows, const void *dout,
                           const uint8_t *relu_mask, const float *relu_scale, const float *relu_shift, const void *y,
                           const float *mean, const float *invstd, const float *gamma, float *dgamma, float *dbeta,
                           void *dy, const float *partial2, const void *y2, const float *mean2, const float *invstd2,
                           const float *gamma2, float *dgamma2, float *dbeta2, void *dy2, int32_t accumulate,
                           float *coef, int64_t M, int32_t C, void *stream);

/* The backward of a downsampling block's two BatchNorms (the block's last BN and its
 * downsample branch's BN, both fed dout * relu_mask): pose6d_bn_bwd_mask for (y, mean,
 * invstd, gamma -> dgamma, dbeta, dy) and for (y2, ... -> dy2), bit for bit, in three
 * launches (one reduce, one finalize, one apply: dout and the mask read once per pass).
 * workspace: 2 * (pose6d_bn_bwd_workspace_rows(M) * 2 + 3) * C floats. */
int pose6d_bn_bwd_mask_dual(int32_t dtype, const void *dout, const uint8_t *relu_mask, const void *y,
                            const float *mean, const float *invstd, const float *gamma, float *dgamma, float *dbeta,
                            void *dy, const void *y2, const float *mean2, const float *invstd2, const float *gamma2,
                            float *dgamma2, float *dbeta2, void *dy2, int32_t accumulate, float *workspace, int64_t M,
                            int32_t C, void *stream);
int pose6d_bn_bwd(int32_t dtype, const void *dout, const void *out, const float *relu_scale,
                  const float *relu_shift, const void *y, const float *mean, const float *invstd, const float *gamma,
                  float *dgamma, float *dbeta, int32_t accumulate, void *dy, void *dz_out, float *workspace,
                  int64_t M, int32_t C, void *stream);

/* conv bias gradient: out[c] (+)= sum_m x[m][c] over an NHWC tensor of M pixels */
int pose6d_channel_sum(int32_t dtype, const void *x, int64_t M, int32_t C, float *out, int32_t accumulate,
                       void *stream);
/* the same sum in two passes (row-block partials in `workspace`, then one add per channel in
 * block order: deterministic) -- for long tensors, where pose6d_channel_sum's one block per
 * 64 channels is serial (32 channels x 400 K pixels: 23 ms against tens of microseconds).
 * Any workspace size works (up to 512 * C floats are used); with room for fewer than two
 * row blocks, or C not a power-of-two number of 16-byte chunks, it is pose6d_channel_sum. */
int pose6d_channel_sum_ws(int32_t dtype, const void *x, int64_t M, int32_t C, float *out, int32_t accumulate,
                          float *workspace, int64_t workspace_floats, void *stream);

/* nn.MaxPool2d(k, s, p) on NHWC; argmax = window index (uint8) of the first max */
int pose6d_maxpool_fwd(int32_t dtype, const void *x, void *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                       int32_t C, int32_t k, int32_t s, int32_t p, int32_t Ho, int32_t Wo, void *stream);
/* pose6d_bn_act_fwd (ReLU, no residual) followed by pose6d_maxpool_fwd in one pass: y, argmax
 * as that pair would produce them (bit for bit), without the full-resolution activation. */
int pose6d_bn_relu_maxpool_fwd(int32_t dtype, const void *x, const float *scale, const float *shift, void *y,
                               uint8_t *argmax, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s,
                               int32_t p, int32_t Ho, int32_t Wo, void *stream);
int pose6d_maxpool_bwd(int32_t dtype, const void *dy, const uint8_t *argmax, void *dx, int32_t N, int32_t H,
                       int32_t W, int32_t C, int32_t k, int32_t s, int32_t p, int32_t Ho, int32_t Wo, void *stream);
/* nn.AdaptiveAvgPool2d(1) + view(B, -1): x [N][HW][C] -> y [N][C] fp32 */
int pose6d_avgpool_fwd(int32_t dtype, const void *x, float *y, int32_t N, int32_t HW, int32_t C, void *stream);
int pose6d_avgpool_bwd(int32_t dtype, const float *dy, void *dx, int32_t N, int32_t HW, int32_t C, void *stream);

/* ------------------------------------------------------------------------
 * Fully-connected heads (fp32) — nn.Linear / BatchNorm1d / ReLU / GELU / Dropout
 * of the rot/trans/z heads (pose_net_rgb.py:23-50, pose_net_rgbd_geometric.py:28-38,
 * pose_net_rgb_geometric.py:23-33,58-65, pose_net_rgbd.py:73-103).
 * ---------------------------------------------------------------------- */
/* C[m][n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias[n]) + beta * C[m][n]
 * workspace (may be NULL): ws_floats fp32 for split-K partials of skinny GEMMs
 * (reduced in fixed order; >= 16 * M * N floats enables the full split). */
int pose6d_gemm_f32(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C,
                    int64_t ldc, const float *bias, int32_t M, int32_t N, int32_t K, float alpha, float beta,
                    float *workspace, int64_t ws_floats, void *stream);
/* eval-mode nn.Linear followed by nn.BatchNorm1d (running statistics) [+ ReLU], one
 * launch path (replaces the rot/trans heads' Linear -> BatchNorm1d -> ReLU of
 * pose_net_rgb.py:27-35 / pose_net_rgbd_geometric.py:28-38 at eval):
 *   C[m][n] = act((A W^T + bias)[m][n] - rmean[n]) * (1 / sqrt(rvar[n] + eps)) * gamma[n] + beta[n])
 * with pose6d_gemm_f32 + pose6d_bn1d_fwd(training = 0)'s arithmetic bit for bit.  A [M][sam]
 * (K used), W [N][K] (nn.Linear weight), batch M <= 32. */
int pose6d_gemm_f32_bn_eval(const float *A, int64_t sam, const float *W, float *C, int64_t ldc, const float *bias,
                            int32_t M, int32_t N, int32_t K, const float *gamma, const float *beta,
                            const float *running_mean, const float *running_var, float eps, int32_t relu,
                            float *workspace, int64_t ws_floats, void *stream);
/* nn.Linear parameter gradients in one launch: dW[n][k] (+)= sum_b dy[b*ldy + n] x[b*ldx + k],
 * db[n] (+)= sum_b dy[b*ldy + n] (db may be NULL); dW [N][K] contiguous. */
int pose6d_linear_wgrad(const float *dy, int64_t ldy, const float *x, int64_t ldx, float *dw, float *db, int32_t N,
                        int32_t K, int32_t B, int32_t accumulate, void *stream);
/* db[n] (+)= sum_m dy[m * ldy + n]  (Linear bias gradient; ldy >= N) */
int pose6d_colsum_f32(const float *dy, int64_t ldy, float *db, int32_t M, int32_t N, int32_t accumulate,
                      void *stream);
/* BatchNorm1d (+ReLU) (+Dropout p_drop with a counter-based RNG keyed by the
 * device word *seed xor salt -- a device word so graph replays draw new masks) */
int pose6d_bn1d_fwd(const float *x, float *y, int32_t M, int32_t C, const float *gamma, const float *beta,
                    float *running_mean, float *running_var, int64_t *num_batches, float momentum, float eps,
                    int32_t training, int32_t relu, float p_drop, const uint64_t *seed, uint64_t salt, uint8_t *mask,
                    float *save_mean, float *save_invstd, void *stream);
int pose6d_bn1d_bwd(const float *dy, const float *x, const float *y, int32_t M, int32_t C, const float *gamma,
                    const float *save_mean, const float *save_invstd, int32_t training, int32_t relu, float p_drop,
                    const uint8_t *mask, float *dx, float *dgamma, float *dbeta, int32_t accumulate, void *stream);
/* act: 0 identity, 1 ReLU, 2 GELU (erf); optional dropout */
int pose6d_act_fwd(const float *x, float *y, int64_t n, int32_t act, float p_drop, const uint64_t *seed,
                   uint64_t salt, uint8_t *mask, void *stream);
int pose6d_act_bwd(const float *dy, const float *x, float *dx, int64_t n, int32_t act, float p_drop,
                   const uint8_t *mask, void *stream);

/* ------------------------------------------------------------------------
 * RGB-D fusion (PoseNetRGBD, pose_net_rgbd.py:66-103,118-142), fp32.
 * LayerNorm over rows of D (nn.LayerNorm(D): biased variance, eps), fused with
 * act (0 none, 1 ReLU, 2 exact GELU) and Dropout(p) — the nn.Sequential runs
 * LayerNorm -> GELU -> Dropout of `fusion` / `rot_head` / `trans_head`
 * (pose_net_rgbd.py:72-103) and rgb_norm / depth_norm (:68-69, :127-128, act 0).
 * Row strides (ld*) let the two normalised features land side by side in the
 * (B, 2D) concatenation (:134) without a copy; y2 (optional, contiguous)
 * receives a second copy.  mean / rstd (B each) are saved for the backward.
 * Backward: dy (+ dy2 when non-null: a second gradient flowing into the same
 * output, e.g. the residual and the concatenation branch) -> dx (+= when
 * accumulate_dx), dgamma / dbeta (+= when accumulate).
 * ---------------------------------------------------------------------- */
int pose6d_layernorm_fwd(const float *x, int64_t ldx, float *y, int64_t ldy, float *y2, int32_t B, int32_t D,
                         const float *gamma, const float *beta, float eps, int32_t act, float p_drop,
                         const uint64_t *seed, uint64_t salt, uint8_t *mask, float *mean, float *rstd,
                         void *stream);
int pose6d_layernorm_bwd(const float *dy, int64_t lddy, const float *dy2, int64_t lddy2, const float *x,
                         int64_t ldx, int32_t B, int32_t D, const float *gamma, const float *beta,
                         const float *mean, const float *rstd, int32_t act, float p_drop, const uint8_t *mask,
                         float *dx, int64_t lddx, int32_t accumulate_dx, float *dgamma, float *dbeta,
                         int32_t accumulate, void *stream);
/* Two independent plain LayerNorms (act 0, no dropout: rgb_norm / depth_norm,
 * pose_net_rgbd.py:127-128) over (B, D) rows in ONE launch each way.  Side a and side b
 * each have their own x / gamma / beta / eps / mean / rstd and their own output pointer
 * and row stride; y2_* (optional, contiguous (B, D)) receives a second copy.  Forward:
 * a grid of 2 B workgroups.  Backward: one grid of 2 B row workgroups (dx_* = the
 * LayerNorm backward of dy_* + dy2_*, dy2_* optional, strides separate; dx is stored,
 * never accumulated) followed by 2 ceil(D / 256) column workgroups (dgamma_* / dbeta_*,
 * += when accumulate); dx, dgamma and dbeta of both sides are required.  Per row and
 * per column the arithmetic is pose6d_layernorm_fwd / pose6d_layernorm_bwd's own (shared
 * device functions): the results equal two separate calls bit for bit.  Every ld >= D;
 * B == 0 returns POSE6D_OK. */
int pose6d_layernorm_pair_fwd(const float *x_a, int64_t ldx_a, float *y_a, int64_t ldy_a, float *y2_a,
                              const float *gamma_a, const float *beta_a, float eps_a, float *mean_a, float *rstd_a,
                              const float *x_b, int64_t ldx_b, float *y_b, int64_t ldy_b, float *y2_b,
                              const float *gamma_b, const float *beta_b, float eps_b, float *mean_b, float *rstd_b,
                              int32_t B, int32_t D, void *stream);
int pose6d_layernorm_pair_bwd(const float *dy_a, int64_t lddy_a, const float *dy2_a, int64_t lddy2_a,
                              const float *x_a, int64_t ldx_a, const float *gamma_a, const float *beta_a,
                              const float *mean_a, const float *rstd_a, float *dx_a, int64_t lddx_a, float *dgamma_a,
                              float *dbeta_a, const float *dy_b, int64_t lddy_b, const float *dy2_b, int64_t lddy2_b,
                              const float *x_b, int64_t ldx_b, const float *gamma_b, const float *beta_b,
                              const float *mean_b, const float *rstd_b, float *dx_b, int64_t lddx_b, float *dgamma_b,
                              float *dbeta_b, int32_t B, int32_t D, int32_t accumulate, void *stream);

/* CrossModalAttention core (pose_net_rgbd.py:23-35): per sample b,
 *   attn = softmax((q_b k_b^T) * scale), q_b, k_b, v_b = (H, hd) views of rows
 *   of the projections; out_b = dropout(attn) v_b, flattened back to H*hd.
 * probs (B*H*H) keeps the pre-dropout softmax for the backward; mask (B*H*H)
 * the dropout draw.  H <= 16. */
int pose6d_xattn_fwd(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H, int32_t hd,
                     float scale, float p_drop, const uint64_t *seed, uint64_t salt, float *probs, uint8_t *mask,
                     void *stream);
int pose6d_xattn_bwd(const float *dout, const float *q, const float *k, const float *v, const float *probs,
                     const uint8_t *mask, int32_t B, int32_t H, int32_t hd, float scale, float p_drop, float *dq,
                     float *dk, float *dv, void *stream);
/* The same kernels with element row strides (each >= H * hd) on q, k, v, out and, in the
 * backward, on dout, q, k, v, dq, dk, dv: k and v (dk and dv) may be the two halves of one
 * (B, 2 H hd) buffer, the output / input of a stacked K|V projection.  The contiguous
 * entry points above call these with every stride H * hd.  probs and mask stay
 * contiguous (B*H*H) and the dropout index stays b*H*H + i*H + j, so one seed and salt
 * draw the same mask whatever the strides. */
int pose6d_xattn_fwd_strided(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv,
                             float *out, int64_t ldo, int32_t B, int32_t H, int32_t hd, float scale, float p_drop,
                             const uint64_t *seed, uint64_t salt, float *probs, uint8_t *mask, void *stream);
int pose6d_xattn_bwd_strided(const float *dout, int64_t lddo, const float *q, int64_t ldq, const float *k,
                             int64_t ldk, const float *v, int64_t ldv, const float *probs, const uint8_t *mask,
                             int32_t B, int32_t H, int32_t hd, float scale, float p_drop, float *dq, int64_t lddq,
                             float *dk, int64_t lddk, float *dv, int64_t lddv, void *stream);

/* ------------------------------------------------------------------------
 * Optimiser — clip_grad_norm_(params, max_norm) + AdamW.step() of the callers
 * (train_rgbd_geometric.py:65,111-112) over one flat fp32 buffer.
 * hp (device) = {lr, beta1, beta2, eps, weight_decay, step t (>= 1; bias
 *                corrections 1 - beta^t computed in-kernel), grad scale (applied to
 *                grad before the norm; 0 reads as 1 — the DDP trainer's 1/world),
 *                max_norm (<= 0: no clipping)}
 * grad, param and both moment buffers must be 16-byte aligned (read as float4).
 * ---------------------------------------------------------------------- */
int pose6d_sumsq_partial(const float *g, int64_t n, float *partials, int32_t nparts, void *stream);
/* the same, and (each optional) step[0] += 1 (the hp[5] counter pose6d_adamw_step reads next) and
 * seed[0] += 1 (the trainer's dropout seed word): the per-step counters without launches of their own */
int pose6d_sumsq_partial_step(const float *g, int64_t n, float *partials, int32_t nparts, float *step,
                              int64_t *seed, void *stream);
int pose6d_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                      const float *partials, int32_t nparts, const float *hp, float *norm_out, void *stream);
/* The same update (bit-identical), that also writes every conv's packed compute-dtype
 * copies (wp / wt of pose6d_pack_conv_weights) from the updated values: the next
 * forward reads them without a packing launch.  Each conv's OIHW master must be a
 * 16-B aligned slice of param; wp's padding entries are never written (pack once,
 * with pose6d_pack_conv_weights, before the first step and after any write to the
 * masters from outside this call).  descs: device copy of the pack table (n_desc
 * records, see pose6d_pack_conv_weights).  jobs: device copy of the int32 [n_jobs][4]
 * work table pose6d_adamw_packed_jobs builds on the host from a HOST copy of the same
 * table (device addresses compared as integers) -- it returns the job count (cap /
 * jobs may be 0 / NULL to size the table), or a negative error code. */
int pose6d_adamw_packed_jobs(const void *descs, int32_t n_desc, const float *param, int64_t n, int32_t *jobs,
                             int32_t cap);
int pose6d_adamw_step_packed(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                             const float *partials, int32_t nparts, const float *hp, float *norm_out, int32_t dtype,
                             const void *descs, const int32_t *jobs, int32_t n_jobs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
