/*
 * mpa_hip.h — C ABI of libmpa_hip.so, the MI355X (gfx950) native operator library for the
 * multi-part-assembly training hot path.
 *
 * Every entry point takes raw DEVICE pointers, plain sizes and a HIP stream handle
 * (`void* stream` == hipStream_t; NULL = the legacy default stream), returns 0 on success or a
 * negative MPA_E* code, never allocates or frees user-visible memory, never synchronises the
 * device, and keeps no mutable global state besides a thread-local last-error string
 * (mpa_last_error).  All launches are asynchronous on `stream`.
 *
 * Each block below cites the reference interface (Wuziyi616/multi_part_assembly, file:line) that
 * the entry point replaces; INTEGRATION.md shows the reference-side binding.
 */
#ifndef MPA_HIP_H_
#define MPA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPA_OK 0
#define MPA_EINVAL (-1)  /* bad argument (null pointer, negative size, size overflow) */
#define MPA_ELAUNCH (-2) /* hipGetLastError() reported a launch failure */

/* ABI version of this header; bumped whenever a signature changes. */
#define MPA_ABI_VERSION 10
int mpa_abi_version(void);

/* Thread-local, NUL-terminated description of the last failure on this thread ("" if none). */
const char* mpa_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Chamfer distance — replaces the `chamfer_cuda` extension module
 *   chamfer_forward : multi_part_assembly/utils/chamfer/cuda/chamfer.cpp:21
 *                     -> ChamferForward   chamfer_kernel.cu:116-168 (kernel :32-95)
 *   chamfer_backward: multi_part_assembly/utils/chamfer/cuda/chamfer.cpp:22
 *                     -> ChamferBackward  chamfer_kernel.cu:224-289 (kernel :175-210)
 *
 * Layout: xyz1 [batch, n1, 3], xyz2 [batch, n2, 3] contiguous fp32 (AoS), as CHECK_INPUT
 * (chamfer_kernel.cu:20-22) demands.  Outputs dist1 [batch, n1], dist2 [batch, n2] fp32 and
 * idx1, idx2 int64 — the dtypes ChamferForward allocates (:129-132).
 *
 * Semantics (bit-exact contract, see DESIGN.md "Chamfer arithmetic"):
 *   d(p,q) = ((px-qx)*(px-qx) + (py-qy)*(py-qy)) + (pz-qz)*(pz-qz), every operation rounded to
 *   fp32, no fused multiply-add; dist1[b,i] = min_j d(xyz1[b,i], xyz2[b,j]) and idx1[b,i] the LOWEST
 *   j attaining it (strict `<` scan in index order, chamfer_kernel.cu:82); a query with no
 *   candidate below 1e32 (n2 == 0, NaN/huge input) gets dist = 1e32f, idx = -1 (:60-61).
 *   dist2/idx2: the same with the roles of the clouds swapped.
 *
 * Three searches stand behind the call, with identical results (tests/test_chamfer_gpu.py, tests/test_gate_gpu.py):
 *   - the exhaustive scan: n1 * n2 pair evaluations per sample and direction (what the reference does);
 *   - the matrix-core gated search (csrc/gate_nn.hip) for clouds of a few hundred to a few thousand points — the per-part
 *     call of rot_points_cd_loss, [B*P, N, 3] against itself (utils/loss.py:113-138): one bf16 matrix instruction per
 *     32 x 32 pairs bounds every pair, the pinned fp32 arithmetic answers from the few candidates that can win.  No
 *     workspace.  Chosen when min(n1, n2) >= 192 and the grid-pruned search below is not;
 *   - an exact grid-pruned search (csrc/grid_nn.hip) for large clouds — the whole-shape call of shape_cd_loss,
 *     [32, 20000, 3] against itself (utils/loss.py:173-199), is 2.56e10 pair evaluations exhaustively and a few
 *     dozen candidates per query pruned.  It needs scratch memory, which the CALLER provides (the library never
 *     allocates): `workspace` = mpa_chamfer_workspace() bytes, 16-byte aligned, contents irrelevant before and
 *     after the call (0 bytes for the sizes the exhaustive scan answers anyway; mpa_chamfer_workspace_variant sizes
 *     a pinned search of mpa_chamfer_forward_variant).  With workspace == NULL (or too small) every size is answered
 *     by the exhaustive scan.
 *   The pruned search is chosen when min(n1, n2) >= 512 and n1 * n2 >= 9e6.  Samples that hold a non-finite
 *   coordinate, or one beyond 1e15 in magnitude, are always answered by the exhaustive scan.
 * ---------------------------------------------------------------------------------------------- */
int mpa_chamfer_workspace(int64_t batch, int64_t n1, int64_t n2, int64_t* bytes);
int mpa_chamfer_workspace_variant(int64_t batch, int64_t n1, int64_t n2, int variant, int64_t* bytes);
int mpa_chamfer_forward(const float* xyz1, const float* xyz2, int64_t batch, int64_t n1, int64_t n2,
                        float* dist1, int64_t* idx1, float* dist2, int64_t* idx2, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Diagnostic twin of mpa_chamfer_forward that pins the search (all bit-identical in their results):
 * 0 = direct compare/select per pair, 1 = fused-form gate + exact recheck (fastest on tie-free clouds),
 * 2 = exact chunk-minimum scan (the exhaustive default: insensitive to duplicated points), 3 = the grid-pruned
 * search at ANY size (needs the workspace), 4 = the matrix-core gated search (any n1, n2 in 1 .. 32768; no workspace),
 * -1 = by size as mpa_chamfer_forward does. */
int mpa_chamfer_forward_variant(const float* xyz1, const float* xyz2, int64_t batch, int64_t n1,
                                int64_t n2, float* dist1, int64_t* idx1, float* dist2,
                                int64_t* idx2, int variant, void* workspace, int64_t workspace_bytes,
                                void* stream);

/*
 * grad_xyz1 [batch, n1, 3] and grad_xyz2 [batch, n2, 3] are OVERWRITTEN (the library zero-fills
 * them itself, as ChamferBackward does with at::zeros, chamfer_kernel.cu:252-253):
 *   grad_xyz1[b,i]        += 2*grad_dist1[b,i] * (xyz1[b,i] - xyz2[b,idx1[b,i]])
 *   grad_xyz2[b,idx1[b,i]] -= the same vector                 (and symmetrically for dist2/idx2)
 * The scatter half uses fp32 hardware atomics, so the summation ORDER of colliding contributions
 * is unspecified — exactly the reference's behaviour (chamfer_kernel.cu:203-208).
 * Indices outside [0, n) (the -1 of an empty search) contribute nothing.
 */
int mpa_chamfer_backward(const float* grad_dist1, const float* grad_dist2, const float* xyz1,
                         const float* xyz2, const int64_t* idx1, const int64_t* idx2, int64_t batch,
                         int64_t n1, int64_t n2, float* grad_xyz1, float* grad_xyz2, void* stream);

/* Double-precision twins (the reference dispatches float and double, chamfer_kernel.cu:145,156,
 * and its own gradcheck runs in double, utils/chamfer/test_chamfer.py:92-101).  Same contract with
 * every fp32 replaced by fp64 (initial distance 1e32 as a double). */
int mpa_chamfer_forward_f64(const double* xyz1, const double* xyz2, int64_t batch, int64_t n1,
                            int64_t n2, double* dist1, int64_t* idx1, double* dist2, int64_t* idx2,
                            void* stream);
int mpa_chamfer_backward_f64(const double* grad_dist1, const double* grad_dist2, const double* xyz1,
                             const double* xyz2, const int64_t* idx1, const int64_t* idx2,
                             int64_t batch, int64_t n1, int64_t n2, double* grad_xyz1,
                             double* grad_xyz2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rigid pose application — replaces the tensor-op chain of
 *   rot_pc / transform_pc : multi_part_assembly/utils/transforms.py:199-244
 *   qrot / qtransform     : multi_part_assembly/utils/transforms.py:75-109
 *   (pytorch3d.transforms.quaternion_apply underneath, transforms.py:87)
 *
 * pc [num_parts, num_points, 3] fp32, quat [num_parts, 4] (real part first, NOT normalised here),
 * trans [num_parts, 3] or NULL (rotation only), mask [num_parts] or NULL: where mask[m] == 0 every
 * point of part m is replaced by (fill, fill, fill) BEFORE the transform — the padded-part fill of
 * shape_cd_loss (utils/loss.py:173-175).  out [num_parts, num_points, 3].
 * Arithmetic: the two Hamilton products of quaternion_apply evaluated term by term, left to right,
 * no FMA — bit-identical to the reference CPU path.
 * ---------------------------------------------------------------------------------------------- */
int mpa_pose_apply_forward(const float* pc, const float* quat, const float* trans,
                           const float* mask, float fill, int64_t num_parts, int64_t num_points,
                           float* out, void* stream);

/* Backward of the above: given grad_out [num_parts, num_points, 3] writes grad_quat [num_parts, 4],
 * grad_trans [num_parts, 3] (skipped if NULL) and grad_pc [num_parts, num_points, 3] (skipped if
 * NULL; zero for masked parts).  Deterministic (fixed reduction tree, no atomics). */
int mpa_pose_apply_backward(const float* grad_out, const float* pc, const float* quat,
                            const float* mask, float fill, int64_t num_parts, int64_t num_points,
                            float* grad_quat, float* grad_trans, float* grad_pc, void* stream);

/* Rotation3D's constructor rule (multi_part_assembly/utils/rotation.py:115-126): quaternions [count, 4] whose
 * norm is <= 0.5 (zero padding) are replaced by the identity (1,0,0,0); keep [count] receives 1 where the input
 * was kept (the gradient gate).  One launch instead of norm + compare + where. */
int mpa_quat_sanitize(const float* quat, int64_t count, float* out, float* keep, void* stream);

/* The weighting of the loss terms for one stochastic sample (multi_part_assembly/models/modules/base_model.py:348-387:
 * `loss = sum_k w_k * mean_b term_k[b]`): terms [K, B] row-major, weights [K] -> means [K] (what the reference logs per
 * term) and loss [1], in ONE launch instead of mean + dot; fixed reduction order.  1 <= K <= 64.
 * Backward: grad_terms [K, B] = (grad_loss[0] * w_k + grad_means[k]) / B; grad_loss and grad_means may each be NULL. */
int mpa_loss_reduce_forward(const float* terms, const float* weights, int64_t K, int64_t B, float* means, float* loss,
                            void* stream);
int mpa_loss_reduce_backward(const float* grad_loss, const float* grad_means, const float* weights, int64_t K, int64_t B,
                             float* grad_terms, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused geometric-assembly loss — replaces, for the geometric datasets, the loss half of
 *   BaseModel._calc_loss : multi_part_assembly/models/modules/base_model.py:240-314
 * i.e. trans_l2_loss, rot_cosine_loss, rot_points_l2_loss, rot_points_cd_loss, shape_cd_loss
 * (utils/loss.py:22-35,59-202) together with their rot_pc / transform_pc / chamfer_distance calls and
 * the autograd graph behind them.  Same values as composing mpa_pose_apply_* and mpa_chamfer_*,
 * without touching padded slots: padded target parts enter the whole-shape search as ONE
 * representative point (all their points coincide after the 1e3 fill), padded query points are
 * skipped (the loss multiplies their distances by zero).
 *
 * part_pcs [B,P,N,3]; valids [B,P] (1/0); quat_* [B,P,4] real-first, already passed through
 * Rotation3D's zero-quaternion rule; trans_* [B,P,3].  P <= 64.
 * losses [5,B]: 0 trans_loss, 1 rot_pt_cd_loss, 2 transform_pt_cd_loss, 3 rot_loss, 4 rot_pt_l2_loss
 * (names of base_model.py:283-298), `training` selects the whole-shape normalisation of
 * utils/loss.py:185-198.  The caller provides the workspaces sized by mpa_assembly_loss_workspace
 * and keeps them untouched until the backward call.  The four transformed clouds are the first
 * 4*B*P*N*3 floats of float_ws: rot(pred), rot(gt), transform(pred), transform(gt), each [B,P,N,3];
 * with fill_pad_points != 0 the padded parts of the last two are filled completely (the `ret_pts`
 * outputs of shape_cd_loss), otherwise only their first point is defined.
 * ---------------------------------------------------------------------------------------------- */
int mpa_assembly_loss_workspace(int64_t B, int64_t P, int64_t N, int64_t* float_elems,
                                int64_t* int_elems);
int mpa_assembly_loss_forward(const float* part_pcs, const float* valids, const float* quat_pred,
                              const float* trans_pred, const float* quat_gt, const float* trans_gt,
                              int64_t B, int64_t P, int64_t N, int training, int fill_pad_points,
                              float* float_ws, int32_t* int_ws, float* losses, void* stream);
/* Profiling twin: identical launches; `events` (may be NULL) is a host array of 7 hipEvent_t recorded on
 * `stream`: [0] start, [1] after pose kernel, [2] after per-part Chamfer, [3] after the whole-shape Chamfer
 * phase, [4] after finalize, [5]/[6] right before/after the whole-shape search kernel itself — so a benchmark can
 * time the dominant kernel inside its timed region.  Individual entries may be NULL (e.g. only [5] and [6] set: two
 * records per call instead of seven). */
int mpa_assembly_loss_forward_timed(const float* part_pcs, const float* valids, const float* quat_pred,
                                    const float* trans_pred, const float* quat_gt, const float* trans_gt,
                                    int64_t B, int64_t P, int64_t N, int training, int fill_pad_points,
                                    float* float_ws, int32_t* int_ws, float* losses, void* const* events,
                                    void* stream);
/* The spatial structure behind both Chamfer searches of the loss.  Every cloud the loss searches — rot_pc / transform_pc of
 * part_pcs under the predicted and the ground-truth pose (utils/loss.py:127-129,177-183) — is a rigid image of the same
 * source points, so ONE balanced k-d ordering of each valid part's N points (leaves of 32) serves them all: it depends on
 * part_pcs and valids only, not on any pose.  mpa_assembly_order writes it (order: mpa_assembly_order_elems floats =
 * [B*P][Npad] x (local x, y, z, original index), Npad = the power of two >= max(N, 32); 0 floats and a no-op when
 * N > 2048, where the loss keeps its grid search); mpa_assembly_loss_forward_ordered is mpa_assembly_loss_forward_timed
 * taking that ordering, so a training step orders its batch once and evaluates the loss as often as the model asks
 * (3 GNN iterations, min-of-N samples).  order == NULL: computed into the workspace by the call itself.  The ordering
 * steers speed only — results are the exhaustive scan's, bit for bit, for any permutation.
 * `search` picks the searches behind the two Chamfer terms (identical results): 0 exhaustive scans, 1 exhaustive per-part
 * scan + grid-pruned whole-shape search (rounds 1-4; the default), 2 k-d leaves for both, 3 "auto" = leaves for the per-part
 * term and, per sample on the device, grid or leaves for the whole-shape term; -1 = MPA_SHAPE_SEARCH (brute | grid | leaf
 * | auto) or the default.  The leaf structure wins where parts are many and small; only modes 2 / 3 use `order`. */
int mpa_assembly_order_elems(int64_t B, int64_t P, int64_t N, int64_t* float_elems);
int mpa_assembly_order(const float* part_pcs, const float* valids, int64_t B, int64_t P, int64_t N, float* order,
                       void* stream);
int mpa_assembly_loss_forward_ordered(const float* part_pcs, const float* valids, const float* quat_pred,
                                      const float* trans_pred, const float* quat_gt, const float* trans_gt,
                                      int64_t B, int64_t P, int64_t N, int training, int fill_pad_points,
                                      const float* order, int search, float* float_ws, int32_t* int_ws, float* losses,
                                      void* const* events, void* stream);
/* grad_losses [5,B] = d(objective)/d(losses); writes grad_quat [B,P,4] and grad_trans [B,P,3] of the
 * PREDICTED pose.  Deterministic (no atomics).  Every row is written.  A padded part takes the gradient the reference gives
 * it: exactly zero unless its fill point R (1e3,1e3,1e3) + t is the nearest predicted point of some valid ground-truth point
 * of its sample (whole-shape term, GT -> prediction direction), and then that term's gradient through the fill point, to
 * its rotation and its translation.  A sample without a valid part: the loss terms that are means over its valid parts are NaN (0 / 0, as
 * the reference gives) -- all but transform_pt_cd_loss with training != 0, which divides by P N and is 0 -- and the
 * gradients of all its parts are exactly zero, whatever grad_losses holds for it.  A stored index of -1
 * (no candidate below 1e32) contributes no gradient. */
int mpa_assembly_loss_backward(const float* grad_losses, const float* part_pcs, const float* valids,
                               const float* quat_pred, const float* trans_pred, const float* quat_gt,
                               const float* trans_gt, int64_t B, int64_t P, int64_t N, int training,
                               const float* float_ws, const int32_t* int_ws, float* grad_quat,
                               float* grad_trans, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet part encoder — replaces
 *   PointNet.forward           : multi_part_assembly/models/modules/encoder/pointnet.py:29-41
 *   _extract_part_feats        : multi_part_assembly/models/pn_transformer/network.py:59-68
 *                                (boolean-mask compaction + scatter; here: mask in, zeros out)
 * 5 x [1x1 conv (no bias) -> BatchNorm1d -> ReLU (none after the last)], widths 3-64-64-64-128-F,
 * max over the N points of every part.  F must be 64, 128 or 256 (the shipped configs use 128 / 256),
 * N <= 32768 points per part (the reference samples 1000 per part and feeds P*N = 20000 to B-Global's shape encoder).
 *
 * points [M,N,3]; valids [M] (1/0): padded parts are skipped everywhere (they do not enter the
 * BatchNorm statistics) and get feat = 0.  conv_w[l] = [C_l, C_{l-1}] row-major (the Conv1d weight
 * with its trailing 1 dropped), bn_w / bn_b / running_mean / running_var [C_l], l = 0..4 — HOST
 * arrays of 5 DEVICE pointers each.  training != 0: batch statistics (biased variance) and running
 * statistics updated in place with `momentum` (unbiased variance), else running statistics.
 * feat [M,F].  Workspaces sized by mpa_pointnet_workspace must stay untouched until backward.
 * A call in which NO part is valid returns zero features, leaves the running statistics untouched and its backward
 * writes zero gradients (the reference's BatchNorm would refuse the empty batch).
 * ---------------------------------------------------------------------------------------------- */
int mpa_pointnet_workspace(int64_t M, int64_t N, int64_t F, int64_t* float_elems, int64_t* int_elems);
int mpa_pointnet_forward(const float* points, const float* valids, const float* const* conv_w,
                         const float* const* bn_w, const float* const* bn_b,
                         float* const* running_mean, float* const* running_var, int training,
                         float momentum, float eps, int64_t M, int64_t N, int64_t F, float* float_ws,
                         int32_t* int_ws, float* feat, void* stream);
/* Training-mode backward: grad_feat [M,F] -> grad_conv_w[l] [C_l, C_{l-1}], grad_bn_w[l], grad_bn_b[l]
 * (host arrays of 5 device pointers; every buffer is overwritten).  No gradient w.r.t. the points.
 * Deterministic: two-stage reductions, no atomics. */
int mpa_pointnet_backward(const float* grad_feat, const float* points, const float* valids,
                          const float* const* conv_w, const float* const* bn_w, int64_t M, int64_t N,
                          int64_t F, float* float_ws, const int32_t* int_ws, float* const* grad_conv_w,
                          float* const* grad_bn_w, float* const* grad_bn_b, void* stream);

/* bf16 PERFORMANCE VARIANT of the PointNet encoder (csrc/pointnet_bf16.hip) — separately named, never the default,
 * outside every parity claim (the reference's own precision switch: AMP runs the encoder's convolutions in half
 * precision and keeps the Chamfer loss in fp32, multi_part_assembly/utils/chamfer/chamfer.py:14).  Same arguments
 * and masking as mpa_pointnet_forward / _backward above; the convolution outputs are STORED in bf16, the GEMMs are
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, BatchNorm statistics / affine / every reduction and all returned
 * gradients are fp32 and deterministic.  One workspace (`bytes` from mpa_pointnet_workspace_bf16, 256-byte aligned)
 * that must stay untouched between forward and backward. */
int mpa_pointnet_workspace_bf16(int64_t M, int64_t N, int64_t F, int64_t* bytes);
int mpa_pointnet_forward_bf16(const float* points, const float* valids, const float* const* conv_w,
                              const float* const* bn_w, const float* const* bn_b, float* const* running_mean,
                              float* const* running_var, int training, float momentum, float eps, int64_t M,
                              int64_t N, int64_t F, void* ws, float* feat, void* stream);
int mpa_pointnet_backward_bf16(const float* grad_feat, const float* points, const float* valids,
                               const float* const* conv_w, const float* const* bn_w, int64_t M, int64_t N, int64_t F,
                               void* ws, float* const* grad_conv_w, float* const* grad_bn_w, float* const* grad_bn_b,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * DGCNN part encoder, whole forward / backward — replaces
 *   DGCNN.forward        : multi_part_assembly/models/modules/encoder/dgcnn.py:73-109 (global_feat = True)
 *   _extract_part_feats  : multi_part_assembly/models/dgl/network.py:90-99 (boolean-mask compaction + scatter; here:
 *                          mask in, zeros out, the valid parts are counted and compacted on the device)
 * 4 x [kNN (k = 20) -> Conv2d 1x1 over [x_j - x_i ; x_i] -> BatchNorm2d -> LeakyReLU 0.2 -> max_k], widths
 * 3-64-64-128-256, concatenation (512) -> Conv1d 1x1 -> BatchNorm1d -> LeakyReLU 0.2 -> [max ; mean] over the N
 * points -> Linear(2F -> F).  20 <= N <= 1024 points per part, F = 64, 128 or 256.
 *
 * points [M,N,3]; valids [M] (1/0): padded parts are skipped everywhere (they do not enter the BatchNorm statistics)
 * and get feat = 0.  conv_w[l]: the Conv2d / Conv1d weights with their trailing 1s dropped, [64,6] [64,128] [128,128]
 * [256,256] [F,512]; bn_w / bn_b / running_mean / running_var [C_l], l = 0..4 — HOST arrays of 5 DEVICE pointers;
 * fc_w [F,2F], fc_b [F].  training != 0: batch statistics (over all edges of the valid parts), running statistics
 * updated in place; else running statistics.  feat [M,F].
 * kNN indices: arithmetic and tie rule pinned as for mpa_knn_exact below (index-exact against oracle/knn_ref.c).
 * `ws` (mpa_dgcnn_workspace bytes, 256-byte aligned) carries everything backward needs and must stay untouched until
 * then.  `events` (nullable): host array of 8 hipEvent_t, [2l] / [2l+1] recorded on `stream` right before / after the
 * kNN kernels of stage l — lets a benchmark time them inside its timed region.
 * backward (training mode): grad_feat [M,F] -> grad_conv_w[l], grad_bn_w[l], grad_bn_b[l] (host arrays of 5 device
 * pointers), grad_fc_w, grad_fc_b (all overwritten) and, if non-NULL, grad_points [M,N,3] (through the edge features;
 * the neighbour choice itself is not differentiable).  Deterministic: no cross-wave atomics on floats.
 * ---------------------------------------------------------------------------------------------- */
int mpa_dgcnn_workspace(int64_t M, int64_t N, int64_t F, int64_t* bytes);
int mpa_dgcnn_forward(const float* points, const float* valids, const float* const* conv_w,
                      const float* const* bn_w, const float* const* bn_b, float* const* running_mean,
                      float* const* running_var, const float* fc_w, const float* fc_b, int training, float momentum,
                      float eps, int64_t M, int64_t N, int64_t F, void* ws, float* feat, void* const* events,
                      void* stream);
/* The same forward with caller-supplied kNN graphs, and the read-out of the graphs a forward built.  `graphs`: HOST array
 * of 4 DEVICE pointers, one per EdgeConv stage; a non-NULL entry [nv*N, 20] int32 (indices inside each cloud, rows of
 * the nv VALID parts in order) replaces that stage's search, a NULL entry is searched as usual.  The reference rebuilds
 * every graph from the features (dgcnn.py:84-96); this entry point exists so that a parity test can hold the graphs
 * fixed to the reference's own `knn` outputs and attribute what remains of a difference.  mpa_dgcnn_export_graph copies
 * stage `stage`'s (0..3) lists out of a forward's workspace: idx [M*N, 20] int32, rows past the valid parts = -1. */
int mpa_dgcnn_forward_graphs(const float* points, const float* valids, const float* const* conv_w,
                             const float* const* bn_w, const float* const* bn_b, float* const* running_mean,
                             float* const* running_var, const float* fc_w, const float* fc_b, int training,
                             float momentum, float eps, int64_t M, int64_t N, int64_t F, void* ws, float* feat,
                             const int32_t* const* graphs, void* stream);
int mpa_dgcnn_export_graph(const void* ws, int64_t M, int64_t N, int64_t F, int64_t stage, int32_t* idx,
                           void* stream);
/* The selections a forward stored for its backward, for parity tests that hold the maxima fixed (read-only on the
 * workspace, rows in the order of mpa_dgcnn_export_graph).  stage 0..3: out [M*N, CO] int32 (CO = 64, 64, 128, 256), the
 * selected neighbour SLOT (0..19) of every point and channel of that EdgeConv stage; stage 4: out [M, F] int32, the point
 * (0..N-1) the max-pooling of the tail took per part and channel.  Rows past the valid parts = -1. */
int mpa_dgcnn_export_selection(const void* ws, int64_t M, int64_t N, int64_t F, int64_t stage, int32_t* out,
                               void* stream);
/* LeakyReLU is the encoder's third discrete choice: the slope the backward takes at every activation it differentiates.
 * stage 0..3: out [M*N, CO] int32, 1 where the stage's stored output is positive (unit slope), 0 where the backward
 * takes the slope 0.2; stage 4: out [M*N, F], the same for the tail's rows.  To be read BEFORE the backward (it
 * overwrites the tail's rows).  Rows past the valid parts = -1. */
int mpa_dgcnn_export_branch(const void* ws, int64_t M, int64_t N, int64_t F, int64_t stage, int32_t* out, void* stream);
int mpa_dgcnn_backward(const float* grad_feat, const float* const* conv_w, const float* const* bn_w,
                       const float* fc_w, int64_t M, int64_t N, int64_t F, void* ws, float* const* grad_conv_w,
                       float* const* grad_bn_w, float* const* grad_bn_b, float* grad_fc_w, float* grad_fc_b,
                       float* grad_points, void* stream);

/* kNN graph with the pinned arithmetic, as used inside mpa_dgcnn_forward — replaces `knn`
 * (multi_part_assembly/models/modules/encoder/dgcnn.py:8-15) for n clouds of N points (20 <= N <= 1024), k = 20.
 * x [n*N, ld] row-major point features (16-byte aligned), the first C columns are used (C = 3: ld = 4 with a zero pad
 * column; C = 64 / 128: any ld >= C, a multiple of 4).  idx [n*N, 20] int32, best first.
 *   C = 3:    dot = fma(x2,y2, fma(x1,y1, x0*y0)), |x|^2 = (x0*x0 + x1*x1) + x2*x2 — the reference's CPU arithmetic,
 *             bit for bit (torch matmul + torch.sum on the fixture cloud);
 *   C >= 64:  dot = fmaf chain over k in the order 0, C/2, 1, C/2+1, ... (the matrix-core chain), |x|^2 likewise;
 *   score = (-|x_j|^2 + 2 dot) - |x_i|^2, every operation rounded to fp32; neighbours = the 20 best by (score
 *   descending, index ascending).  On the reference's own stage inputs this selects exactly the reference's neighbour
 *   sets (tests/golden/dgcnn_graphs.npz).
 * C >= 64 runs as a shortlist search (csrc/dg_knn_fast.h): bf16 matrix-core Gram tiles with a proven error bound select
 * ~21 of the N candidates per point, only those get the pinned fp32 score — same indices as the exhaustive scan, bit for
 * bit.  `ws`: mpa_knn_exact_workspace(n, N) bytes of scratch, 256-byte aligned. */
int mpa_knn_exact_workspace(int64_t n, int64_t N, int64_t* bytes);
int mpa_knn_exact(const float* x, int64_t ld, int64_t n, int64_t N, int64_t C, void* ws, int32_t* idx,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * One MLP layer of the graph networks — replaces the Conv1d(k=1) + BatchNorm1d + ReLU layers of
 *   MLP3 / MLP4 / MLP5   : multi_part_assembly/models/dgl/modules.py:5-58, models/rgl_net/modules.py:5-30
 * and the Linear + ReLU layers of
 *   RelationNet          : multi_part_assembly/models/dgl/modules.py:61-73
 * which DGL / RGL-NET run over the B*P*P part pairs (edge MLP, relation weights) and the B*P parts (node MLP) in every
 * GNN iteration (models/dgl/network.py:121-152).
 * x [R, K] row-major (leading dimension ldx >= K), w [N, K] (the Conv1d weight with its trailing 1 dropped / the Linear
 * weight), bias [N] or NULL; gamma == NULL: out = act(x w^T + bias); else out = act(BatchNorm(x w^T + bias)) with
 * batch statistics over the R rows (training != 0; running statistics updated in place) or the running statistics.
 * act = ReLU if relu != 0.  K and N multiples of 64.  out [R, N].  `ws` (mpa_mlp_layer_workspace bytes, 256-byte
 * aligned) carries the pre-normalisation values and the statistics to backward, which takes the forward's `out`
 * (for the ReLU mask) and overwrites grad_x [R, K] (if non-NULL), grad_w [N, K], grad_b [N] (if non-NULL),
 * grad_gamma / grad_beta [N] (BatchNorm layers).  Exact-fp32 matrix-core GEMMs, fixed-order reductions: deterministic.
 * ---------------------------------------------------------------------------------------------- */
int mpa_mlp_layer_workspace(int64_t R, int64_t K, int64_t N, int64_t* bytes);
int mpa_mlp_layer_forward(const float* x, int64_t ldx, const float* w, const float* bias, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, int training, float momentum,
                          float eps, int relu, int64_t R, int64_t K, int64_t N, void* ws, float* out, void* stream);
int mpa_mlp_layer_backward(const float* grad_out, const float* x, int64_t ldx, const float* w, const float* gamma,
                           const float* out, int relu, int64_t R, int64_t K, int64_t N, void* ws, float* grad_x,
                           float* grad_w, float* grad_b, float* grad_gamma, float* grad_beta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * First layer of the P x P edge MLP without the pair tensor — replaces, for the edge MLP's first Conv1d(k=1) + BatchNorm1d
 * + ReLU, the reference's
 *   torch.cat([part_feats.unsqueeze(2).repeat(..), part_feats.unsqueeze(1).repeat(..)], dim=-1) -> MLP3.conv1 / bn1 / relu
 *   (multi_part_assembly/models/dgl/network.py:135-152, models/dgl/modules.py:5-31; RGL-NET: models/rgl_net/network.py:70-88).
 * The layer's input row (s, i, j) is [a[s, i] ; b[s, j]], so x w^T = (a Wa^T + bias)[s, i] + (b Wb^T)[s, j] with
 * Wa | Wb the column halves of w [N, 2F]: two GEMMs over the B*P part rows instead of one over the B*P*P pair rows, the
 * BatchNorm statistics taken over all B*P*P rows as the reference's BatchNorm1d does.
 * a, b [B*P, F] row-major, w [N, 2F], bias [N] or NULL, gamma / beta / running_* [N] (the layer has a BatchNorm);
 * out [B*P*P, N], row (s, i, j) at (s*P + i)*P + j.  F and N multiples of 64.  `ws`: mpa_pair_layer_workspace bytes,
 * 256-byte aligned, carried from forward to backward, which overwrites grad_a / grad_b [B*P, F] (each if non-NULL;
 * grad_b == grad_a — one tensor in both roles, as the networks call it — receives the sum of the two),
 * grad_w [N, 2F], grad_bias [N] (if non-NULL), grad_gamma / grad_beta [N].  Fixed-order reductions: deterministic.
 * ---------------------------------------------------------------------------------------------- */
int mpa_pair_layer_workspace(int64_t B, int64_t P, int64_t F, int64_t N, int64_t* bytes);
int mpa_pair_layer_forward(const float* a, const float* b, const float* w, const float* bias, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int training, float momentum,
                           float eps, int relu, int64_t B, int64_t P, int64_t F, int64_t N, void* ws, float* out,
                           void* stream);
int mpa_pair_layer_backward(const float* grad_out, const float* a, const float* b, const float* w, const float* gamma,
                            const float* out, int relu, int64_t B, int64_t P, int64_t F, int64_t N, void* ws, float* grad_a,
                            float* grad_b, float* grad_w, float* grad_bias, float* grad_gamma, float* grad_beta,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * The small per-iteration pieces of the graph networks between the MLP layers — replace the library element-wise /
 * reduction / 1-column GEMM launches behind
 *   PoseEncoder.mlp1 + ReLU (7 -> 256)                  : multi_part_assembly/models/dgl/modules.py:76-86
 *   RelationNet.mlp3 + sigmoid, times the valid matrix  : models/dgl/modules.py:61-73, models/dgl/network.py:121-133
 *   the relation-weighted mean of the edge features     : models/dgl/network.py:135-152
 *   the [part i ; part j] pair rows fed to the edge MLP / relation net : models/dgl/network.py:121-125, 135-141
 * narrow_linear_relu: out [R, N] = relu(x [R, K] w[N, K]^T + bias), K <= 16; backward takes the forward's `out` (ReLU
 *   mask) and scratch `ws` (mpa_narrow_linear_relu_workspace floats) and overwrites grad_x [R, K] (if non-NULL),
 *   grad_w [N, K], grad_b [N] (if non-NULL).
 * relation_head: out [R] = sigmoid(h [R, K] . w [K] + bias[0]) * mask [R] (mask NULL = ones), K a multiple of 4; `ws`
 *   (mpa_relation_head_workspace floats) carries the sigmoids to backward, which overwrites grad_h [R, K] (if non-NULL),
 *   grad_w [K], grad_b [1] (if non-NULL).
 * relation_mean: out [G, C] = sum_j edge [G, P, C] rel [G, P] / (sum_j rel [G, P] + 1e-6), P <= 64; backward overwrites
 *   grad_edge [G, P, C] and grad_rel [G, P] (each if non-NULL).
 * pair_rows: out [S, P, P, 2F] = [a [S, P, F] of part i ; b [S, P, F] of part j] for every pair (i, j) (swap != 0: [b of
 *   part j ; a of part i]) — the input rows of the edge MLP and the relation net; F a multiple of 4; backward overwrites
 *   grad_a = sum over j of a's F columns and grad_b = sum over i of b's (each if non-NULL).
 * Fixed-order reductions, no atomics: deterministic.
 * ---------------------------------------------------------------------------------------------- */
int mpa_pair_rows_forward(const float* a, const float* b, int64_t S, int64_t P, int64_t F, int swap, float* out,
                          void* stream);
int mpa_pair_rows_backward(const float* grad_out, int64_t S, int64_t P, int64_t F, int swap, float* grad_a, float* grad_b,
                           void* stream);
int mpa_narrow_linear_relu_forward(const float* x, const float* w, const float* bias, int64_t R, int64_t K, int64_t N,
                                   float* out, void* stream);
int mpa_narrow_linear_relu_workspace(int64_t R, int64_t K, int64_t N, int64_t* float_elems);
int mpa_narrow_linear_relu_backward(const float* grad_out, const float* out, const float* x, const float* w, int64_t R,
                                    int64_t K, int64_t N, float* ws, float* grad_x, float* grad_w, float* grad_b,
                                    void* stream);
int mpa_relation_head_workspace(int64_t R, int64_t K, int64_t* float_elems);
int mpa_relation_head_forward(const float* h, const float* w, const float* bias, const float* mask, int64_t R, int64_t K,
                              float* ws, float* out, void* stream);
int mpa_relation_head_backward(const float* grad_out, const float* h, const float* w, const float* mask, int64_t R,
                               int64_t K, float* ws, float* grad_h, float* grad_w, float* grad_b, void* stream);
int mpa_relation_mean_forward(const float* edge, const float* rel, int64_t G, int64_t P, int64_t C, float* out,
                              void* stream);
int mpa_relation_mean_backward(const float* grad_out, const float* edge, const float* rel, const float* out, int64_t G,
                               int64_t P, int64_t C, float* grad_edge, float* grad_rel, void* stream);
/* Merging of equivalent parts (DGLModel._merge_nodes, multi_part_assembly/models/dgl/network.py:75-88,101-119; no host
 * copy of the ids, no Python loop).  Slots p and q of a sample are equivalent when valids [B,P] is 1 at both and
 * part_ids [B,P] (int32) agree.  Forward, both tensors in one launch: part_out [B,P,C1] / pose_out [B,P,C2] = channel-wise
 * max of part_feats / pose_feats over the slots equivalent to p (padded slots and single-member classes pass through:
 * a pure max, bit-equal to the host loop); arg_part / arg_pose (uint8, same shapes; P <= 64) = the slot the value came
 * from, the LOWEST one on ties (torch's max(dim) on the host picks the same).  Backward: grad_part [B,P,C1] / grad_pose
 * [B,P,C2] at slot q = the sum, in ascending p, of the output gradients of the slots p whose recorded arg is q.  No
 * atomics: deterministic.  Valid parts are expected first in every sample, as the datasets lay them out (the reference
 * indexes the compacted valid list). */
int mpa_merge_equal_parts(const float* part_feats, const float* pose_feats, const float* valids, const int32_t* part_ids,
                          int64_t B, int64_t P, int64_t C1, int64_t C2, float* part_out, float* pose_out,
                          uint8_t* arg_part, uint8_t* arg_pose, void* stream);
int mpa_merge_equal_parts_backward(const float* grad_part_out, const float* grad_pose_out, const uint8_t* arg_part,
                                   const uint8_t* arg_pose, const float* valids, const int32_t* part_ids, int64_t B,
                                   int64_t P, int64_t C1, int64_t C2, float* grad_part, float* grad_pose, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Recurrent half of a single-layer (bi)directional GRU — replaces the per-step library launches behind
 *   RNNWrapper(nn.GRU(batch_first, bidirectional)) : multi_part_assembly/models/modules/rnn.py:6-46
 *   RGLNet.forward                                 : multi_part_assembly/models/rgl_net/network.py:118-127
 * The input projections gi[d][b][t] = W_ih x + b_ih [D,B,T,3H] (gate order r, z, n as torch.nn.GRU) are one GEMM done by
 * the caller; this runs the T sequential steps of D directions in ONE launch:
 *   r = sigmoid(gi_r + W_hr h + b_hr), z = sigmoid(gi_z + W_hz h + b_hz), n = tanh(gi_n + r (W_hn h + b_hn)),
 *   h' = (1 - z) n + z h,   out [D,B,T,H] = h' of every step.
 * h0 [D,B,H], whh [D,3H,H], bhh [D,3H].  H = 128 or 256, B <= 64, D = 1 or 2.  `ws` (mpa_gru_workspace floats)
 * (8-byte aligned) carries the gates to backward and the tagged words the blocks exchange once per step.  backward: grad_out [D,B,T,H] -> grad_gi [D,B,T,3H], grad_whh, grad_bhh (overwritten);
 * deterministic (partials summed in block order, no float atomics).  Sequences of different lengths: run the padded
 * batch (valid steps first) and mask the outputs — the reverse direction on the per-sample reversed valid prefix.
 * ---------------------------------------------------------------------------------------------- */
int mpa_gru_workspace(int64_t D, int64_t B, int64_t T, int64_t H, int64_t* float_elems);
/* *ok = 1 iff the shapes are instantiated AND the current device can hold the whole grid of both kernels at once (their
 * blocks poll for each other's per-step words; forward / backward return an error instead of stalling when it cannot). */
int mpa_gru_resident(int64_t D, int64_t B, int64_t H, int* ok);
/* `status` (device memory, one int32 the caller keeps at 0; NULL: the kernel traps instead): raised to 1 by a launch whose
 * blocks could not all wait for each other — a block that was never dispatched because another stream's kernels (a
 * collective beside the step, say) held its CU makes the waiting blocks give up after a few seconds (MPA_GRU_POLL_BUDGET
 * polls of ~1 us; default 2^22).  The launch then ends on its own with undefined outputs; the caller reads the word when
 * it next synchronises (gru.py raises a RuntimeError from it) — no trap, no hang, the HIP context stays usable. */
int mpa_gru_forward(const float* gi, const float* h0, const float* whh, const float* bhh, int64_t D, int64_t B, int64_t T,
                    int64_t H, float* ws, float* out, int32_t* status, void* stream);
int mpa_gru_backward(const float* grad_out, const float* h0, const float* whh, const float* out, int64_t D, int64_t B,
                     int64_t T, int64_t H, float* ws, float* grad_gi, float* grad_whh, float* grad_bhh, int32_t* status,
                     void* stream);
/* ------------------------------------------------------------------------------------------------
 * B-LSTM seq2seq decoder (live layer 0 of nn.GRU(128, 528, 2 layers) + its output head) — replaces the per-part loop of
 *   Seq2Seq.infer_decoder / DecoderRNN.forward : multi_part_assembly/models/b_lstm/seq2seq.py:106-137,165-191
 * All T steps in ONE launch per pass (same exchange, status word and co-residency rules as mpa_gru_*):
 *   h_t = GRU(gi_t, h_{t-1}) (torch.nn.GRU's equations, H = 528),  z1_t = W1 h_t + b1 [256],  y_t = W2 z1_t + b2 [128].
 * gi [T,B,3H] = W_ih x_t + b_ih of the teacher-forced inputs (one GEMM by the caller), or NULL for free running: then
 * x_0 = 0 and x_t = mask[t] * y_{t-1} (mask [T,B,128] holds the caller's scaled dropout mask, NULL = none), with y_{t-1}
 * exactly the y the launch returns.  h0 [B,H]; wih [3H,128], bih, whh [3H,H], bhh, w1 [256,H], b1, w2 [128,256], b2.
 * Outputs hs [T,B,H], z1 [T,B,256], y [T,B,128]; `ws` (mpa_seq2seq_decoder_workspace floats, 8-byte aligned) carries the
 * gates to backward.  backward: dh [T,B,H] (the head's gradient w.r.t. h_t) -> dgi [T,B,3H] (w.r.t. gi), dwhh, dbhh
 * (overwritten) and dh0 [B,H]; deterministic (partials summed in block order).  B <= 64.
 * ---------------------------------------------------------------------------------------------- */
int mpa_seq2seq_decoder_workspace(int64_t B, int64_t T, int64_t* float_elems);
/* *ok = 1 iff the current device can hold the whole grid of both decoder kernels at once. */
int mpa_seq2seq_decoder_resident(int64_t B, int* ok);
int mpa_seq2seq_decoder_forward(const float* gi, const float* mask, const float* h0, const float* wih, const float* bih,
                                const float* whh, const float* bhh, const float* w1, const float* b1, const float* w2,
                                const float* b2, int64_t B, int64_t T, float* ws, float* hs, float* z1, float* y,
                                int32_t* status, void* stream);
int mpa_seq2seq_decoder_backward(const float* dh, const float* h0, const float* whh, const float* hs, int64_t B,
                                 int64_t T, float* ws, float* dgi, float* dwhh, float* dbhh, float* dh0, int32_t* status,
                                 void* stream);
/* mpa_seq2seq_decoder_forward_sel: the forward with the mode read ON THE DEVICE.  `teacher` (int32 [1], device memory,
 * written by an earlier launch of the same stream — mpa_seq2seq_draw) picks it: nonzero = teacher forcing, the launch is
 * bit-equal to mpa_seq2seq_decoder_forward with the same gi; zero = free running, bit-equal to it with gi = NULL and the
 * same mask.  gi and teacher are always given (NULL: MPA_EINVAL), mask as for free running.  Every block reads the word
 * once in front of its step loop; nothing else about the launch changes (same grid, exchange, workspace, status word), so
 * one captured launch serves both outcomes of the coin.  Backward is mpa_seq2seq_decoder_backward. */
int mpa_seq2seq_decoder_forward_sel(const float* gi, const float* mask, const int32_t* teacher, const float* h0,
                                    const float* wih, const float* bih, const float* whh, const float* bhh,
                                    const float* w1, const float* b1, const float* w2, const float* b2, int64_t B,
                                    int64_t T, float* ws, float* hs, float* z1, float* y, int32_t* status, void* stream);
/* mpa_seq2seq_draw (csrc/seq2seq_draw.hip): the per-forward draws of the seq2seq module in one launch — what the
 * reference draws on the host with np.random.normal, random.random() and LockedDropout's bernoulli_ (seq2seq.py:165-220,
 * 226-241).  multi_part_assembly_amd/seq2seq_draw_ref.py restates the definition in numpy.
 *   Randomness: Philox4x32-10, stateless.  key = (seed low word, seed high word); counter = (i, 0x73320000 | kind, c low
 * word, c high word), c = (counter_dev != NULL ? *counter_dev : counter) + salt (mod 2^64), with counter / counter_dev /
 * salt as in mpa_match_sample_indices.  Word 1 of the counter is one no other user of the generator produces (the list
 * is at mpa_epoch_order).  u24(w) = float(w >> 8) * 2^-24, exact, in [0, 1).
 *   teacher [1] int32: kind 0, block i = 0, word 0 = w: teacher = u24(w) < ratio (float32 comparison) — ratio >= 1 always
 * forces, ratio <= 0 never does; the meaning of `random.random() < ratio`.
 *   noise [B,16] float32: kind 1, block i = 0 .. 4 B - 1 with words (w0, w1, w2, w3) gives elements 4 i .. 4 i + 3 of the
 * flat array by Box-Muller: from a word pair (wa, wb), u1 = (float(wa >> 9) + 0.5f) * 2^-23 (exact, in (0, 1)), u2 =
 * u24(wb), r = sqrtf(-2 logf(u1)), the pair is (r cosf(a), r sinf(a)) with a = float32(2 pi) * u2 rounded to float32;
 * (w0, w1) gives elements 4 i, 4 i + 1 and (w2, w3) elements 4 i + 2, 4 i + 3.  The accurate library logf / sincosf.
 *   mask [T,B,128] float32, or NULL (outside training mode: not drawn): kind 2, flat element e takes word e % 4 of block
 * i = e / 4; value = u24(w) >= p ? 1.0f / (1.0f - p) : 0.0f, the quotient rounded once to float32.
 *   Every byte of every non-NULL output is written on every call; no memset / memcpy nodes: capturable.
 *   MPA_EINVAL (before any launch, no device needed): B outside [1, 64], T outside [1, 4096] (checked with or without a
 * mask), p outside [0, 1) or NaN, NULL noise or teacher. */
int mpa_seq2seq_draw(int64_t B, int64_t T, float p, float ratio, uint64_t seed, uint64_t counter,
                     const uint64_t* counter_dev, uint64_t salt, float* noise, int32_t* teacher, float* mask,
                     void* stream);
/* Test support: `blocks` workgroups that each hold `lds_bytes` of LDS and do nothing for `usec` microseconds — CUs no other
 * stream can use meanwhile (how tests/test_gru_gpu.py provokes the co-residency failure above). */
int mpa_debug_occupy(int64_t blocks, int64_t lds_bytes, int64_t usec, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Part-relation transformer encoder — replaces
 *   TransformerEncoder.forward : multi_part_assembly/models/pn_transformer/transformer.py:63-79
 *   (nn.TransformerEncoder of pre-LN nn.TransformerEncoderLayer, ReLU FFN, batch_first,
 *    src_key_padding_mask = ~valid, final LayerNorm; transformer.py:20-39)
 * tokens [B,P,D] (P <= 64 parts), valid [B*P] (a part is real iff its entry == 1, the reference's
 * `part_valids == 1`; every other part is masked as a KEY; its own row is still computed, as upstream).  D and FF multiples of 64, head dim D/H <= 64, L <= 16 layers.
 * params: HOST array of 12*L + 2 DEVICE pointers, per layer in nn.TransformerEncoderLayer's
 * named_parameters() order — self_attn.in_proj_weight [3D,D], in_proj_bias [3D], out_proj.weight [D,D],
 * out_proj.bias [D], linear1.weight [FF,D], linear1.bias [FF], linear2.weight [D,FF], linear2.bias [D],
 * norm1.weight, norm1.bias, norm2.weight, norm2.bias [D] — then the final norm.weight, norm.bias [D].
 * dropout_p in [0,1) applies to the 4 dropout sites of every layer (attention probabilities, attention
 * output, FFN hidden, FFN output) with a counter-based generator keyed by (seed, site, element): backward
 * must receive the same seed.  seed_dev (nullable): DEVICE address of the seed, read by the kernels instead of
 * `seed` — lets a captured HIP graph draw fresh masks on every replay (the host updates the word between replays).
 * dropout_p = 0 for evaluation.  ws (mpa_transformer_workspace floats) carries the
 * saved activations from forward to backward.  out [B,P,D].
 * backward: grad_out [B,P,D] -> grad_tokens [B,P,D] and grad_params (same layout as params; every buffer
 * is overwritten).  Deterministic: fixed-order reductions, no atomics.
 * ---------------------------------------------------------------------------------------------- */
int mpa_transformer_workspace(int64_t B, int64_t P, int64_t D, int64_t H, int64_t FF, int64_t L,
                              int64_t* float_elems);
int mpa_transformer_forward(const float* tokens, const float* valid, const float* const* params, int64_t B,
                            int64_t P, int64_t D, int64_t H, int64_t FF, int64_t L, float dropout_p,
                            uint64_t seed, const uint64_t* seed_dev, float* ws, float* out, void* stream);
int mpa_transformer_backward(const float* grad_out, const float* valid, const float* const* params, int64_t B,
                             int64_t P, int64_t D, int64_t H, int64_t FF, int64_t L, float dropout_p,
                             uint64_t seed, const uint64_t* seed_dev, float* ws, float* grad_tokens,
                             float* const* grad_params, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose head — replaces
 *   PoseRegressor.forward : multi_part_assembly/models/modules/regressor.py:50-68
 *   (Linear F-256, LeakyReLU 0.2, Linear 256-128, LeakyReLU 0.2, rot_head 128-4 + F.normalize,
 *    trans_head 128-3; regressor.py:33-48)
 * x [M,F] (1 <= F <= 4096: widths that are not a multiple of 64 — labels / noise appended to the features — are
 * zero-padded inside the workspace; M = B*P tokens).  params: HOST array of 8 DEVICE pointers — fc_layers.0.weight
 * [256,F], .bias, fc_layers.2.weight [128,256], .bias, rot_head.weight [4,128], .bias, trans_head.weight
 * [3,128], .bias.  rot [M,4] unit quaternions (x / max(|x|, 1e-12)), trans [M,3].
 * ws (mpa_pose_head_workspace floats) carries activations to backward, which overwrites grad_x [M,F] and
 * the 8 grad_params buffers (fc_layers.0.weight must be unchanged between the two calls).
 * ---------------------------------------------------------------------------------------------- */
int mpa_pose_head_workspace(int64_t M, int64_t F, int64_t* float_elems);
int mpa_pose_head_forward(const float* x, const float* const* params, int64_t M, int64_t F, float* ws,
                          float* rot, float* trans, void* stream);
int mpa_pose_head_backward(const float* grad_rot, const float* grad_trans, const float* x,
                           const float* const* params, int64_t M, int64_t F, float* ws, float* grad_x,
                           float* const* grad_params, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused optimiser step — replaces torch.optim.Adam / AdamW as configured by
 *   BaseModel.configure_optimizers : multi_part_assembly/models/modules/base_model.py:389-406
 * One streaming pass over flat, 16-byte-aligned fp32 buffers of `numel` elements (parameters,
 * gradients, first and second moments).  `step` is the 1-based step count (bias correction),
 * `grad_scale` multiplies the gradient first (1/world_size of the data-parallel mean),
 * `decoupled_weight_decay` selects AdamW (p *= 1 - lr*wd) over Adam's L2 form (g += wd*p).
 * `decay_mask` (nullable = decay everything): [numel] 1/0 per element; the reference's AdamW parameter groups
 * exempt biases and normalisation weights (multi_part_assembly/utils/utils.py:90-125 filter_wd_parameters).
 * ---------------------------------------------------------------------------------------------- */
int mpa_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  int decoupled_weight_decay, int64_t step, float grad_scale, const float* decay_mask,
                  void* stream);

/* Graph-capturable twin: `hyper` is an 8-float DEVICE buffer
 *   [0] lr  [1] 1-beta1^step  [2] sqrt(1-beta2^step)  [3] grad_scale  [4] step count (int32 bits)
 *   [5] clip coefficient (1 = no clipping; written by mpa_grad_clip_coef)  [6] clipped norm (info)  [7] unused.
 * Every call first ADVANCES the step count on the device and recomputes [1], [2] from it, then applies the update:
 * the launch arguments stay constant across replays of a captured step and the host uploads nothing per step (it
 * writes [0] / [3] only when the schedule or the world size changes, [4] when a checkpoint is loaded). */
int mpa_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                      float* hyper, float beta1, float beta2, float eps, float weight_decay,
                      int decoupled_weight_decay, const float* decay_mask, void* stream);

/* Global-norm gradient clipping — replaces Lightning's `gradient_clip_val` (scripts/train.py:90 passes
 * cfg.optimizer.clip_grad; algorithm "norm" = torch.nn.utils.clip_grad_norm_): coef[0] = min(1, max_norm /
 * (|scale * grad|_2 + 1e-6)), coef[1] = that norm; `scale` = *grad_scale_dev if non-NULL else grad_scale (the
 * 1/world of the data-parallel mean that the optimiser applies later).  Point `coef` at hyper + 5 of
 * mpa_adam_step_dev to fold the clipping into the update.  Deterministic two-stage sum in double; `ws` =
 * mpa_grad_clip_workspace bytes. */
int mpa_grad_clip_workspace(int64_t* bytes);
int mpa_grad_clip_coef(const float* grad, int64_t numel, float max_norm, const float* grad_scale_dev,
                       float grad_scale, void* ws, float* coef, void* stream);

/* ---- Guarded optimiser step: a non-finite gradient or a failed launch skips the step ON THE DEVICE -----------------
 * Stands where Lightning's GradScaler stands in the reference's documented `--fp16` runs (docs/model.md:76,95,123): a
 * step whose gradients hold an inf or NaN is dropped, not applied.  Opt-in; the unguarded entry points above are
 * untouched.  No allocation, no synchronisation, launch configurations depend on sizes only (capturable).
 *
 * mpa_step_guard: ONE pass over `grad` (mpa_grad_clip_coef's two-stage double sum, same operations in the same order,
 * which also finds the smallest flat index of a NaN / +-inf element) and ONE one-wave launch whose lane 0 writes
 *   hyper[5], hyper[6]: for a finite gradient and max_norm > 0 the exact bits mpa_grad_clip_coef writes; max_norm <= 0
 *                       = no clipping: hyper[5] = 1, hyper[6] still the norm; non-finite gradient: 1 and +inf;
 *   the verdict:        bit 0 = some element of `grad` is NaN or +-inf (decided from the double sum of squares, which is
 *                       finite exactly when every element is: 2^31 squares of the largest float stay in range — 3e38
 *                       does not trip); bit 1 = `launch_status` is non-NULL and *launch_status != 0;
 *   the step advance:   ONLY for verdict 0, what mpa_adam_step_dev's advance does to hyper[1], hyper[2], hyper[4].
 * `guard`: eight int32 DEVICE words owned by the caller (zero them to start counting)
 *   [0] this call's verdict   [1] steps applied   [2] steps skipped   [3] skipped in a row (0 after an applied step)
 *   [4] flat index of the first non-finite element of the most recent skipped step, -1 if the status word alone
 *   [5] 1-based attempt number ([1] + [2]) of the most recent skipped step, 0 if none   [6] OR of all verdicts   [7] 0.
 * numel = 0 (grad may be NULL) gives verdict 0 unless the status word is raised; numel < 2^31.  `ws` =
 * mpa_step_guard_workspace bytes, 8-byte aligned; `grad` 16-byte aligned.  Restated in numpy by
 * multi_part_assembly_amd/guard_ref.py.
 *
 * mpa_adam_step_guarded: mpa_adam_step_dev WITHOUT its advance launch, behind mpa_step_guard: guard[0] != 0 -> every
 * block returns before its first store (parameters, moments and `hyper` keep their bits); otherwise the same update on
 * the same operands, bit-equal to mpa_adam_step_dev.
 *
 * mpa_guard_mark: one tiny launch in front of a data-parallel all-reduce: *launch_status != 0 -> grad[0] = quiet NaN,
 * else nothing is touched.  A rank-local failure so becomes a non-finite reduced gradient, and with it the same verdict,
 * on every rank, without another collective.
 *
 * mpa_guard_commit: behind mpa_step_guard (and the update), ONE launch over two caller-owned byte ranges of equal size,
 * `live` (every module buffer of the model, optim.BufferSlab) and `shadow` (their bits at the end of the last applied
 * step).  guard[0] == 0 (the step was applied): shadow <- live; guard[0] != 0 (the step was skipped): live <- shadow.
 * The verdict is read from device memory by every block with one uniform load, never passed by value: a captured launch
 * takes the right direction on every replay.  A bitwise copy of `bytes` bytes in 16-byte units (one 16-byte load and
 * one 16-byte store per unit, grid-stride): NaN payloads, -0 and int64 counters pass through unchanged, and nothing
 * outside the two ranges is written.  bytes % 16 == 0, both ranges 16-byte aligned and disjoint; bytes == 0 is a no-op
 * without a launch (the ranges may then be NULL).  `guard` NULL or misaligned, a NULL range with bytes > 0, a misaligned
 * or overlapping range, a negative size or one that is no multiple of 16: MPA_EINVAL, nothing is launched.  Restated by
 * guard_ref.commit.
 *
 * What a skipped step leaves behind.  With mpa_guard_commit behind every guarded step (Trainer(guard_buffers=True)) every
 * module buffer — BatchNorm running statistics, num_batches_tracked, whatever else a module registers — has the bits it
 * had before the skipped step.  Without it they keep what the skipped step's forward wrote.  Never rolled back, and
 * harmless: the dropout-seed positions (host counters; the skipped step's masks are spent, the next step draws fresh
 * ones), the matching and seq2seq draw counters (rewritten from the host counter in front of every step) and the
 * producers' counters (the data stream is outside the step).  The remaining hole: a step whose gradient is finite while a
 * statistic overflowed to inf is APPLIED, and the statistic is committed; only the checkpoint's refusal of non-finite
 * buffers catches that one. */
int mpa_step_guard_workspace(int64_t* bytes);
int mpa_step_guard(const float* grad, int64_t numel, float max_norm, const float* grad_scale_dev, float grad_scale,
                   const int32_t* launch_status, void* ws, float* hyper, int32_t* guard,
                   float beta1, float beta2, void* stream);
int mpa_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                          const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                          int decoupled_weight_decay, const float* decay_mask, const int32_t* guard, void* stream);
int mpa_guard_mark(const int32_t* launch_status, float* grad, int64_t numel, void* stream);
int mpa_guard_commit(const int32_t* guard, void* live, void* shadow, int64_t bytes, void* stream);

/* ---- Exponential moving average of the weights (csrc/weight_average.hip; opt-in) ------------------------------
 * The reference keeps one copy of the weights; this adds the averaged copy of timm's ModelEmaV2 /
 * torch.optim.swa_utils.AveragedModel, kept on the device: e <- e + (1 - d)(p - e) behind every APPLIED optimiser step.
 *
 * mpa_ema_update: ONE launch over both state ranges of a model.
 *   (a) `param` (read) and `ema` (read / written): `numel` float32 elements of the flat parameter buffer; numel % 4 == 0,
 *       both 16-byte aligned and disjoint.
 *   (b) `live` (read) and `ema_state` (read / written): `state_bytes` bytes of the buffer slab (optim.BufferSlab);
 *       state_bytes % 16 == 0, both 16-byte aligned and disjoint.  `segments`: DEVICE table of `num_segments` int64
 *       triples {byte offset, byte size, kind}, one per buffer, `segments_host` the same table in host memory (read
 *       during the call, which is how the table is checked without touching the device; the caller keeps the two
 *       equal).  A segment's slot is [offset, offset + size rounded up to 16); slots start on 16-byte boundaries, ascend,
 *       do not overlap and lie inside the slab.  kind 1: `size` / 4 float32 words averaged like the parameters
 *       (size % 4 == 0); kind 0: copied bit for bit (int64 counters, flags).  The slot's bytes behind `size` are copied
 *       too (BufferSlab pads with zeros).  Nothing outside the slots is written; a zero-size segment writes nothing.
 *       state_bytes == 0 or num_segments == 0 is legal (the pointers may then be NULL).  One block walks one segment:
 *       meant for slabs of many small buffers (BatchNorm statistics), not for one buffer of many megabytes.
 *   `hyper`: the optimiser's eight device words (mpa_adam_step_dev); t = the int32 in hyper[4], read by the kernel BEHIND
 *   this step's advance, so t >= 1.  Every operation below is one rounded float32 operation, no FMA contraction:
 *       a = (float)t;   q = (1 + a) / (10 + a);   d = warmup ? fminf(decay, q) : decay;   c = 1 - d
 *       e = e + c * (p - e)                         (non-finite values propagate as IEEE 754 says)
 *   0 <= decay < 1; warmup 0 / 1.  `guard`: the eight guard words of mpa_step_guard, or NULL; guard[0] != 0 -> every
 *   block returns before its first store (the average of a skipped step keeps its bits).  Verdict and step count are
 *   read from device memory by every block with one uniform load each, never passed by value: a captured launch follows
 *   them on every replay.  Grid-stride, 16 bytes per lane per access, no atomics, no LDS, bit-identical from run to run.
 *   MPA_EINVAL, with nothing launched: a null `hyper`, a null range of non-zero size, a misaligned pointer, numel < 0 or
 *   numel % 4, state_bytes < 0 or state_bytes % 16, decay outside [0, 1) or NaN, overlapping ranges, a segment that is
 *   not 16-byte aligned, leaves the slab, overlaps its predecessor or has an unknown kind.
 *
 * mpa_ema_swap: bitwise exchange, in 16-byte units and ONE launch, of `param` <-> `ema` (`param_bytes` bytes) and
 *   `live` <-> `ema_state` (`state_bytes` bytes).  Two calls give every bit back, NaN payloads and padding included.  Sizes
 *   are non-negative multiples of 16 (zero in either pair, or both, is legal: the pair's pointers may be NULL); ranges
 *   16-byte aligned and pairwise disjoint, else MPA_EINVAL.  It is how averaged weights are put in front of the model:
 *   parameters and buffers stay views of the same memory.
 * Restated in numpy by multi_part_assembly_amd/ema_ref.py. */
int mpa_ema_update(const float* param, float* ema, int64_t numel, const void* live, void* ema_state, int64_t state_bytes,
                   const int64_t* segments_host, const int64_t* segments, int64_t num_segments, const float* hyper,
                   float decay, int warmup, const int32_t* guard, void* stream);
int mpa_ema_swap(void* param, void* ema, int64_t param_bytes, void* live, void* ema_state, int64_t state_bytes,
                 void* stream);

/* ---- Gradient accumulation (csrc/grad_accumulate.hip; opt-in) -------------------------------------------------
 * One optimiser step over a WINDOW of several micro-batches, Lightning's `accumulate_grad_batches`.  The HIP backward
 * kernels overwrite their slices of the flat gradient, so the window's sum is kept in a second flat buffer of the same
 * length, the accumulator, by ONE streaming launch behind every micro-batch's backward:
 *   mode 0 FIRST  acc[i]  = grad[i]            (a copy; the accumulator's old content is never read; 8 B per element)
 *   mode 1 ADD    acc[i]  = acc[i] + grad[i]   (12 B)
 *   mode 2 LAST   grad[i] = acc[i] + grad[i]   (12 B; the sum lands in the flat GRADIENT, so the all-reduce, mpa_guard_mark,
 *                                               mpa_step_guard, the clipping, the Adam kernels, mpa_guard_commit and
 *                                               mpa_ema_update run unchanged on the buffer they already know)
 * A window of k >= 2 micro-batches is FIRST, ADD x (k - 2), LAST and leaves ((g0 + g1) + g2) + ... in `grad`; a window of
 * one micro-batch needs no call.  The mean (1 / k, and 1 / world) is the optimiser's grad_scale.  Every addition is one
 * rounded fp32 operation, denormals are kept, the buffer a mode does not write keeps its bytes.
 *   `mode` is taken by value when `mode_dev` is NULL; otherwise the launch reads the int32 DEVICE word `mode_dev` (one
 *   uniform load), so a launch captured in a graph follows the word on every replay; a word outside 0..2 writes nothing.
 *   Grid: a float4 per lane, grid-stride, at most 2048 blocks of 256; no LDS, no scratch.  numel == 0: success, no launch.
 *   MPA_EINVAL: numel < 0 or numel % 4, a NULL or not 16-byte aligned buffer when numel > 0, overlapping buffers, `mode`
 *   outside 0..2 when mode_dev is NULL, a misaligned mode_dev.
 * Restated in numpy by multi_part_assembly_amd/accum_ref.py. */
int mpa_grad_accumulate(float* grad, float* acc, int64_t numel, int mode, const int32_t* mode_dev, void* stream);

/* ---- GT <-> prediction matching of equivalent parts (semantic datasets) --------------------------------------
 * Replaces BaseModel._linear_sum_assignment / _match_parts (multi_part_assembly/models/modules/base_model.py:
 * 150-238: p x p Chamfer cost matrix on n = 100 sub-sampled points, scipy.optimize.linear_sum_assignment on the
 * host, GT poses permuted inside every group) with device code for all groups of a batch, no host round trip.
 *
 * mpa_linear_sum_assignment: `problems` square cost matrices cost [problems, ld, ld] (float32, the top-left
 *   sizes[i] x sizes[i] block of each is the problem, ld <= 64) -> col4row [problems, ld] (column assigned to each
 *   row, -1 past the size).  scipy's shortest-augmenting-path algorithm (rectangular_lsap.cpp, scipy 1.15.3)
 *   step by step in float64: same assignment as scipy, ties included.
 * mpa_match_parts: match_ids [B,P] int32 (0 = unique or padded, g >= 1 = group g; G = number of group slots
 *   considered, groups with id > G are left unmatched), sample_idx [B,G,n] int32 point indices (the reference
 *   draws torch.randperm(N)[:n] per group), poses as [B,P,3] / [B,P,4] (w,x,y,z).  Writes new_trans / new_quat
 *   (the GT poses after rearrangement), perm [B,P] (source slot of every slot), and leaves the cost matrices
 *   [B,G,P,P] and assignments [B,G,P] in the two workspaces.  A caller that cannot read the ids on the host (a captured
 *   step) passes the static bound G = max(1, P / 2): groups have at least two members and the datasets number them
 *   consecutively from 1, so no id exceeds it; slots of groups a sample does not have cost an empty block each. */
int mpa_linear_sum_assignment(const float* cost, const int32_t* sizes, int64_t problems, int64_t ld,
                              int32_t* col4row, void* stream);
int mpa_match_parts(const float* part_pcs, const float* pred_trans, const float* pred_quat, const float* gt_trans,
                    const float* gt_quat, const int32_t* match_ids, const int32_t* sample_idx, int64_t B, int64_t P,
                    int64_t N, int64_t G, int64_t n, float* cost_ws, int32_t* col4row_ws, float* new_trans,
                    float* new_quat, int32_t* perm, void* stream);
/* mpa_match_parts_rmat: mpa_match_parts with rotation matrices [B,P,3,3] (rot_type='rmat') in place of quaternions: the
 *   clouds of the cost matrices are transformed as in mpa_pose_apply_rmat_forward; new_rmat [B,P,3,3]. */
int mpa_match_parts_rmat(const float* part_pcs, const float* pred_trans, const float* pred_rmat, const float* gt_trans,
                         const float* gt_rmat, const int32_t* match_ids, const int32_t* sample_idx, int64_t B, int64_t P,
                         int64_t N, int64_t G, int64_t n, float* cost_ws, int32_t* col4row_ws, float* new_trans,
                         float* new_rmat, int32_t* perm, void* stream);
/* mpa_match_sample_indices (csrc/match_sample.hip): the sample_idx [B,G,n] int32 of mpa_match_parts drawn on the device.
 *   Row (b, g) holds the first n entries of a uniformly random permutation of 0..N-1 — what the reference's
 *   `torch.randperm(N)[:n]` means — for every group slot, whether the sample has that group or not (the matching
 *   kernels skip empty slots).  1 <= n <= min(N, 128), N <= 16384 (the permutation lives in LDS as 16-bit words; it is
 *   never written to global memory), B * G <= 2^24; anything else: MPA_EINVAL.
 *   Partial Fisher-Yates shuffle: perm = iota(N); for k = 0 .. n-1: j = k + mulhi32(w_k, N - k) (the high 32 bits of the
 *   32 x 32-bit product), swap perm[k] and perm[j], emit perm[k].  mulhi32 picks j uniformly up to a relative bias below
 *   N / 2^32 (< 4e-6 at the cap) per step.
 *   Randomness: Philox4x32-10, stateless.  key = (seed low word, seed high word); w_k = word (k & 3) of the block with
 *   counter = (slot, 0x6D610000 | (k >> 2), c low word, c high word), slot = b * G + g, c = (counter_dev != NULL ?
 *   *counter_dev : counter) + salt (mod 2^64).  Word 1 of the counter is never below 4, the mesh sampler's (see
 *   mpa_mesh_sample_batch) always is: equal seeds give unrelated streams.  `counter` numbers the caller's steps; `salt`
 *   tells the calls of one step apart (the caller passes k * an odd constant for its k-th call).  A captured HIP graph
 *   passes counter_dev, a DEVICE word the host rewrites between replays, so that every replay draws afresh; an eager call
 *   passes the same number by value and draws the same rows. */
int mpa_match_sample_indices(int64_t B, int64_t G, int64_t N, int64_t n, uint64_t seed, uint64_t counter,
                             const uint64_t* counter_dev, uint64_t salt, int32_t* sample_idx, void* stream);

/* ---- batch producer (device side) -------------------------------------------------------------------------
 * Replaces the per-part numpy work of GeometryPartDataset.__getitem__ (multi_part_assembly/datasets/
 * geometry_data.py:74-107,133-146) for a whole batch: raw [M,N,3] float64 sampled points (M = B*max_num_part
 * slots), rot [M,9] float64 row-major rotation matrices, perm [M,N] int32 point orders, valids [M] ->
 * part_pcs [M,N,3] float32 = ((rot @ (p - centroid))[perm]) and part_trans [M,3] float32 = centroid; padded
 * slots are zero-filled.  float64 arithmetic like the reference, fixed summation order. */
int mpa_part_batch_transform(const double* raw, const double* rot, const int32_t* perm, const float* valids,
                             int64_t M, int64_t N, float* part_pcs, float* part_trans, void* stream);

/* Geometry batches sampled from device-resident meshes (csrc/mesh_sample.hip): one launch draws, for each of the M =
 * B * max_num_part slots, N surface samples of part slot_part[m] and runs the transform of mpa_part_batch_transform on
 * them without the float64 cloud leaving LDS (N <= 2048).  The mesh store: tri [F_total,9] float64 = per triangle
 * (origin, e1 = v1 - v0, e2 = v2 - v0), cum_area [F_total] float64 = per part the running sum of its triangle areas,
 * part_face_off [parts_total + 1] int64.  slot_part [M] int64; a negative entry is a padded slot, written as zeros.
 * Per point i, from three uniforms (u0, u1, u2) in [0, 1): pick = u0 * cum[last]; face = first index of the part's
 * segment with cum[face] >= pick; (a, b) = (u1, u2), replaced by (|a - 1|, |b - 1|) where a + b > 1; p = (e1 * a +
 * e2 * b) + origin, each operation rounded once.  Outputs part_pcs [M,N,3], part_trans [M,3] float32 and, if raw_out is
 * not NULL, the sampled float64 cloud raw_out [M,N,3].
 *   Replay mode (uniforms != NULL): uniforms [M,N,3] float64, rot [M,9] float64, perm [M,N] int32 come from the caller;
 * part_pcs and part_trans are bit-equal to mpa_part_batch_transform on the cloud numpy computes from the same uniforms.
 * part_quat may be NULL (the caller knows its rotations); seed, stream_id and rot_range are ignored.
 *   Device-random mode (uniforms, rot, perm all NULL): Philox4x32-10, stateless.  key = (seed low word, seed high word);
 * counter = (i, purpose, stream_id[m] low word, high word).  purpose 0 and 1 are the point draws: u0 = words 0-1 and u1 =
 * words 2-3 of call 0, u2 = words 0-1 of call 1; purpose 2 and 3 with i = 0 are the slot's rotation: r0 = words 0-1 and
 * r1 = words 2-3 of call 2, r2 = words 0-1 of call 3.  A uniform from the word pair (hi, lo), hi the first word, is
 * ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53.  rot_range <= 0: the rotation is the unit quaternion (x, y, z, w) =
 * (sqrt(1-r0) sin 2 pi r1, sqrt(1-r0) cos 2 pi r1, sqrt(r0) sin 2 pi r2, sqrt(r0) cos 2 pi r2) (Shoemake: uniform);
 * rot_range > 0: Euler angles (r - 0.5) * 2 * rot_range degrees, extrinsic xyz.  part_quat [M,4] float32 receives the
 * scalar-first quaternion of the INVERSE rotation.  The points keep their draw order (no permutation).
 *   MPA_EINVAL: negative sizes, N outside [1, 2048], a NULL pointer the mode needs, rot / perm without uniforms. */
int mpa_mesh_sample_batch(const double* tri, const double* cum_area, const int64_t* part_face_off, int64_t parts_total,
                          const int64_t* slot_part, int64_t M, int64_t N, const double* uniforms, const double* rot,
                          const int32_t* perm, uint64_t seed, const int64_t* stream_id, double rot_range,
                          float* part_pcs, float* part_trans, float* part_quat, double* raw_out, void* stream);
/* mpa_mesh_slot_table (csrc/mesh_sample.hip): the slot tables of mpa_mesh_sample_batch for B shapes whose indices
 * shape_index [B] int64 live in DEVICE memory, from the store's shape_part_off [S+1] int64.  For slot m = b * P + j with
 * p = the part count of shape shape_index[b]: slot_part [B*P] int64 = shape_part_off[s] + j for j < p, -1 otherwise;
 * stream_id [B*P] int64 = stream_base + m (mod 2^64); valids [B*P] float32 = 1 for j < p, else 0; part_ids [B*P] float32 =
 * j for j < p, else 0 — what datasets.DeviceGeometryProducer builds on the host from host indices.
 *   Checked at run time, because they come from device memory: a shape index outside [0, S) reads nothing from
 * shape_part_off and stores 1 into the device word `status`; a part count outside [min_part, max_part] stores 2.  Either
 * way all P slots of that shape are padded (slot_part -1, valids 0).  The kernel never clears `status`.
 *   MPA_EINVAL (before any launch): negative B / S, B > 2^24, P outside [1, 4096], limits that do not satisfy 0 <= min_part
 * <= max_part <= P, a NULL pointer.  B == 0 with valid sizes is MPA_OK. */
int mpa_mesh_slot_table(const int64_t* shape_part_off, int64_t S, const int64_t* shape_index, int64_t B, int64_t P,
                        int64_t min_part, int64_t max_part, uint64_t stream_base, int64_t* slot_part,
                        int64_t* stream_id, float* valids, float* part_ids, int32_t* status, void* stream);

/* ---- the sample order of an epoch (csrc/epoch_order.hip) --------------------------------------------------------------
 * Replaces torch.randperm + DistributedSampler behind the reference's loaders (multi_part_assembly/datasets/
 * geometry_data.py:226-248, scripts/train.py:57-120) with two launches; multi_part_assembly_amd/sampler_ref.py restates
 * the definition in numpy.
 *   key_i, i = 0..S-1, is the 64-bit word x | (y << 32) of the Philox4x32-10 block with key = (seed low word, seed high
 * word) and counter = (i, 0x65700000, e low word, e high word), e = (epoch_dev != NULL ? *epoch_dev : epoch) as an unsigned
 * 64-bit number.  Word 1 of the counter is one no other user of the generator produces (mpa_mesh_sample_batch: below 4;
 * mpa_match_sample_indices: 0x6D61xxxx; mpa_partnet_gather_batch: 0x706Exxxx; mpa_seq2seq_draw: 0x7332xxxx), so equal seeds
 * give unrelated streams.
 *   perm = 0..S-1 sorted ascending by (key_i, i): a stable argsort, ties cannot make it ambiguous.
 *   Sharding as torch.utils.data.DistributedSampler(shuffle=True, drop_last=False): total = ceil(S / world) * world;
 * padded[q] = perm[q mod S] for q < total (perm followed by its first total - S entries, repeated where world > 2 S);
 * out [total / world] int64 = padded[rank], padded[rank + world], padded[rank + 2 world], ...  Every rank computes the same
 * permutation from (seed, e): no communication.  Exactly total / world entries of `out` are written.
 *   A captured HIP graph passes epoch_dev, a DEVICE word the host rewrites between replays.  Deterministic: ranks are
 * counted (rank_i = the number of j with (key_j, j) < (key_i, i), S^2 comparisons against LDS tiles), every entry is
 * written once, no atomics; no memset / memcpy nodes: capturable.
 *   workspace: mpa_epoch_order_workspace(S) bytes (8 S: the keys), 8-byte aligned, caller-owned.  S <= 2^18 = 262144.
 *   MPA_EINVAL (before any launch, no device needed): S <= 0, world outside [1, 2^20], rank outside [0, world), S above
 * the maximum, a NULL or misaligned workspace, NULL out. */
int mpa_epoch_order_workspace(int64_t S, int64_t* bytes);
int mpa_epoch_order(int64_t S, int64_t world, int64_t rank, uint64_t seed, int64_t epoch, const int64_t* epoch_dev,
                    void* workspace, int64_t* out, void* stream);

/* PartNet batches gathered from a device-resident store (csrc/partnet_gather.hip): one launch writes the whole data_dict
 * of PartNetPartDataset.__getitem__ + default collate (multi_part_assembly/datasets/partnet_data.py:127-243) for B shapes.
 *   The store (datasets.PartNetStore validates it when it is built; the kernel trusts it): pcs [parts_total,N,3], poses
 * [parts_total,7] (translation, then scalar-first quaternion), sym [parts_total,3] float32; geo_ids, sem_ids
 * [parts_total] int32 (geo_part_ids >= 0; the files' 1-based part_ids); shape_part_off [S+1] int64 (shape s owns the parts
 * shape_part_off[s] .. shape_part_off[s+1]-1, their number p_s <= P); shape_ids [S] int64; optional contacts
 * [sum_s p_s^2, 4] float32 with contact_off [S+1] int64 in rows of 4 (shape s: its p_s x p_s x 4 block, row-major).
 *   shape_index [B] int64 in DEVICE memory selects the shapes.  P = max_num_part in [1, 64], N points per part, C =
 * num_part_category (0: part_label is zero-width and not written).
 *   Part order of sample b, a permutation `order` of 0..p-1 (slot j holds stored part start + order[j]):
 *     - perm == NULL and random_order == 0: the identity;
 *     - replay, perm [B,P] int32 != NULL: order[j] = perm[b,j] for j < p (the rest of the row is ignored);
 *     - device-random, random_order != 0: a full Fisher-Yates shuffle of iota(p): for k = 0 .. p-2: j = k + mulhi32(w_k,
 *       p - k) (the high 32 bits of the 32 x 32-bit product), swap order[k] and order[j].  Philox4x32-10, stateless: key =
 *       (seed low word, seed high word); w_k = word (k & 3) of the block with counter = (b, 0x706E0000 | (k >> 2), c low
 *       word, c high word), c = (counter_dev != NULL ? *counter_dev : counter).  Word 1 of the counter is one neither
 *       other user of the generator produces (mpa_mesh_sample_batch: below 4; mpa_match_sample_indices: 0x6D61xxxx).  A
 *       captured HIP graph passes counter_dev, a DEVICE word the host rewrites between replays.
 *   Outputs, one pointer per key, NULL = not produced; every byte of every other one is written on every call (nothing
 * relies on an earlier fill).  For slot (b, j) with j < p and part = start + order[j]: part_pcs [B,P,N,3] = the cloud,
 * part_trans [B,P,3] / part_quat [B,P,4] = the pose split, sym_out [B,P,3]; slots j >= p are zeros.  From the ordered ids
 * g_j = geo_ids[part]: part_valids [B,P] (1 for j < p); part_ids [B,P] = g_j as float32; instance_label [B,P,P] = one-hot
 * at the number of i < j with g_i == g_j; match_ids [B,P] float32: ids >= 1 that occur at least twice are numbered 1, 2, ..
 * in ascending id value, every other slot is 0; part_label [B,P,C] = one-hot at sem_ids[part] - 1 (an id above C gives a
 * zero row); valid_matrix [B,P,P] = valids outer valids; shape_id [B] int64 = shape_ids[shape_index[b]].
 * contact_points [B,P,P,4] is the stored p x p x 4 block zero-padded and stays in STORED part order even when the parts
 * are shuffled or replayed: the reference reads the contact file after its shuffle and does not permute it.
 * order_out [B,P] int32 (debugging, tests): the order used, -1 in padded slots.
 *   Checked at run time, because they come from device memory: a shape_index outside [0, S) reads nothing from the store,
 * is written as an all-padding sample (valids 0, shape_id -1) and stores 1 into the device word `status`; a replay row
 * whose first p entries are not a permutation of 0..p-1 is treated the same way with status 2.  The kernel never clears
 * `status` (the caller does, after reading it).  No input makes the kernel read outside the store.
 *   The cloud moves with 16-byte accesses when N % 4 == 0 and pcs / part_pcs are 16-byte aligned, with dword accesses
 * otherwise.  One launch, no atomics, no memset / memcpy nodes: capturable.
 *   MPA_EINVAL (before any launch): P outside [1, 64]; negative or oversized B, S, N, C; perm together with random_order;
 * contact_points requested from a store without contacts (contacts or contact_off NULL); NULL shape_part_off /
 * shape_index / status; a requested output whose store array is NULL.  B == 0 with valid sizes is MPA_OK. */
int mpa_partnet_gather_batch(const float* pcs, const float* poses, const float* sym, const int32_t* geo_ids,
                             const int32_t* sem_ids, const int64_t* shape_part_off, const int64_t* shape_ids,
                             const float* contacts, const int64_t* contact_off, int64_t S, const int64_t* shape_index,
                             int64_t B, int64_t P, int64_t N, int64_t C, const int32_t* perm, int32_t random_order,
                             uint64_t seed, uint64_t counter, const uint64_t* counter_dev, float* part_pcs,
                             float* part_trans, float* part_quat, float* part_valids, float* part_ids,
                             float* instance_label, float* match_ids, float* part_label, float* contact_points,
                             float* sym_out, float* valid_matrix, int64_t* shape_id, int32_t* order_out, int32_t* status,
                             void* stream);

/* ---- rotation matrices (rot_type='rmat'; csrc/rmat.hip, the 6D pose head in csrc/transformer.hip) -------------------------
 * Replaces the rmat half of multi_part_assembly/utils/rotation.py:134-167 and utils/transforms.py:126-244, and the 6D
 * branch of models/modules/regressor.py:6-27,33-69.  Matrices are [.., 3, 3] row-major fp32.
 *
 * mpa_quat_to_rmat: pytorch3d quaternion_to_matrix of quat [count, 4] (real part first; |q|^2 summed left to right) ->
 *   rmat [count, 9].  No backward (it converts ground-truth poses).
 * mpa_rot6d_to_rmat_forward: pytorch3d rotation_6d_to_matrix of rot6d [count, 6] -> rmat [count, 9]: rows b1 =
 *   normalize(a1), b2 = normalize(a2 - (b1.a2) b1) (F.normalize: x / max(|x|, 1e-12)), b3 = b1 x b2.
 *   _backward: grad_rmat [count, 9] -> grad_rot6d [count, 6].
 * mpa_pose_apply_rmat_forward / _backward: the contract of mpa_pose_apply_* with rmat [num_parts, 9] in place of quat:
 *   out_i = (r_i0 x + r_i1 y) + r_i2 z (+ t_i), left to right, no FMA (the reference's `r @ v[..., None]`).  Backward:
 *   grad_rmat [num_parts, 9] = sum_n g p^T, grad_trans (NULL: skipped), grad_pc = R^T g (NULL: skipped; zero where
 *   masked).  Deterministic (fixed reduction tree, no atomics).
 * mpa_pose_head6_*: mpa_pose_head_* with the 6D rotation head: params[4] = rot.w [6,128], params[5] = rot.b [6];
 *   rot6d [M, 6] = normalize_rot6d(h . Wr^T + br) (reference regressor.py:6-27), trans [M, 3].  Its own workspace size. */
int mpa_quat_to_rmat(const float* quat, int64_t count, float* rmat, void* stream);

/* The fused assembly loss (mpa_assembly_loss_*) with rotation matrices: rmat_pred / rmat_gt [B,P,3,3] row-major in place
 * of the quaternions, same workspace (mpa_assembly_loss_workspace), same searches and routes, same outputs.  Padded
 * parts and samples without a valid part take the gradients documented at mpa_assembly_loss_backward.  The clouds
 * are transformed as in mpa_pose_apply_rmat_forward; rot_loss = mean over the nine entries of (I - R1^T R2)^2
 * (utils/loss.py:76-82); the backward writes grad_rmat [B,P,3,3] as fixed-order sums dL/dR = sum g p^T plus the closed
 * form of rot_loss (no atomics, deterministic). */
int mpa_assembly_loss_forward_rmat(const float* part_pcs, const float* valids, const float* rmat_pred,
                                   const float* trans_pred, const float* rmat_gt, const float* trans_gt, int64_t B,
                                   int64_t P, int64_t N, int training, int fill_pad_points, float* float_ws,
                                   int32_t* int_ws, float* losses, void* stream);
int mpa_assembly_loss_forward_rmat_timed(const float* part_pcs, const float* valids, const float* rmat_pred,
                                         const float* trans_pred, const float* rmat_gt, const float* trans_gt,
                                         int64_t B, int64_t P, int64_t N, int training, int fill_pad_points,
                                         float* float_ws, int32_t* int_ws, float* losses, void* const* events,
                                         void* stream);
int mpa_assembly_loss_forward_rmat_ordered(const float* part_pcs, const float* valids, const float* rmat_pred,
                                           const float* trans_pred, const float* rmat_gt, const float* trans_gt,
                                           int64_t B, int64_t P, int64_t N, int training, int fill_pad_points,
                                           const float* order, int search, float* float_ws, int32_t* int_ws,
                                           float* losses, void* const* events, void* stream);
int mpa_assembly_loss_backward_rmat(const float* grad_losses, const float* part_pcs, const float* valids,
                                    const float* rmat_pred, const float* trans_pred, const float* rmat_gt,
                                    const float* trans_gt, int64_t B, int64_t P, int64_t N, int training,
                                    const float* float_ws, const int32_t* int_ws, float* grad_rmat, float* grad_trans,
                                    void* stream);
int mpa_rot6d_to_rmat_forward(const float* rot6d, int64_t count, float* rmat, void* stream);
int mpa_rot6d_to_rmat_backward(const float* rot6d, const float* grad_rmat, int64_t count, float* grad_rot6d,
                               void* stream);
int mpa_pose_apply_rmat_forward(const float* pc, const float* rmat, const float* trans, const float* mask, float fill,
                                int64_t num_parts, int64_t num_points, float* out, void* stream);
int mpa_pose_apply_rmat_backward(const float* grad_out, const float* pc, const float* rmat, const float* mask,
                                 float fill, int64_t num_parts, int64_t num_points, float* grad_rmat,
                                 float* grad_trans, float* grad_pc, void* stream);
int mpa_pose_head6_workspace(int64_t M, int64_t F, int64_t* float_elems);
int mpa_pose_head6_forward(const float* x, const float* const* params, int64_t M, int64_t F, float* ws,
                           float* rot6d, float* trans, void* stream);
int mpa_pose_head6_backward(const float* grad_rot6d, const float* grad_trans, const float* x,
                            const float* const* params, int64_t M, int64_t F, float* ws, float* grad_x,
                            float* const* grad_params, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics of one batch (csrc/eval_metrics.hip) — replace the composition behind
 *   BaseModel._calc_metrics : multi_part_assembly/models/modules/base_model.py:316-339
 *   calc_part_acc, trans_metrics, rot_metrics, calc_connectivity_acc : multi_part_assembly/utils/eval_utils.py:12-199
 *
 * mpa_assembly_metrics[_rmat]: part_pcs [B, P, N, 3], trans_pred / trans_gt [B, P, 3], rotations as the Rotation3D
 * value holds them — quaternions [B, P, 4] (real part first, not normalised) or row-major matrices [B, P, 3, 3] —
 * valids [B, P] (1 = real part, 0 = padding), all contiguous fp32.  out [7, B] receives, in this order,
 *   part_acc, trans_mse, trans_rmse, trans_mae, rot_mse, rot_rmse, rot_mae
 * and per_part [B, P] (NULL to skip) the per-part Chamfer value mean_i dist1 + mean_j dist2 between the part posed by
 * the predicted and by the ground-truth pose (0 for padded slots).  The posed coordinates are those of
 * mpa_pose_apply[_rmat]_forward and the nearest-neighbour distances those of mpa_chamfer_forward, bit for bit; the
 * two means are summed in a fixed shape of at most 20 fp32 roundings (relative error <= 1.2e-6).  part_acc counts the
 * valid parts with per_part < 0.01 over the valid parts.  The translation / Euler-angle ('zyx', degrees, wrapped at
 * 180) errors are evaluated in float64 from the fp32 inputs, weighted by valids and divided by their sum (the
 * reference's `_valid_mean`; no valid part -> NaN, as the reference gives), rounded to fp32 once.
 * Two launches, no atomics, fixed reduction order: bit-identical from run to run.  Padded slots (valids == 0) are
 * never read: any values in their points and poses leave every output bit unchanged.
 * Envelope: 1 <= N <= 2048 (both posed clouds of a part live in LDS, 24 N bytes), P >= 1, 7 * B * P < 2^31, finite
 * inputs (a non-finite coordinate of a valid part makes its distances undefined).  Outside it the call is refused
 * with MPA_EINVAL and the caller composes the metrics from the operators above.
 * workspace: mpa_assembly_metrics_workspace() bytes, 8-byte aligned, contents irrelevant before and after.
 *
 * mpa_connectivity_acc: contact_points [B, P, P, 4] (flag, x, y, z), trans [B, P, 3], rot [B, P, 4] or [B, P, 3, 3]
 * (is_rmat != 0).  For every (b, i, j) with flag == 1: the minimum squared distance between the 8 sign-flipped copies
 * of contact_points[b, i, j, 1:] posed by part i and the 8 of contact_points[b, j, i, 1:] posed by part j; out [B] is
 * (contacts with minimum < 0.01) / contacts in every element, NaN without contacts.  One launch of one block,
 * integer counters only.  B * P * P < 2^31.
 * ---------------------------------------------------------------------------------------------- */
int mpa_assembly_metrics_workspace(int64_t B, int64_t P, int64_t* bytes);
int mpa_assembly_metrics(const float* part_pcs, const float* trans_pred, const float* trans_gt, const float* quat_pred,
                         const float* quat_gt, const float* valids, int64_t B, int64_t P, int64_t N, void* workspace,
                         float* out, float* per_part, void* stream);
int mpa_assembly_metrics_rmat(const float* part_pcs, const float* trans_pred, const float* trans_gt,
                              const float* rmat_pred, const float* rmat_gt, const float* valids, int64_t B, int64_t P,
                              int64_t N, void* workspace, float* out, float* per_part, void* stream);
int mpa_connectivity_acc(const float* contact_points, const float* trans, const float* rot, int is_rmat, int64_t B,
                         int64_t P, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Assembled shapes for export (csrc/assemble.hip) -- replace the tail of
 *   BaseModel.sample_assembly : multi_part_assembly/models/modules/base_model.py:427-460 (+ utils/utils.py:49-64)
 * and the mesh half of scripts/vis.py:75-96.
 *
 * mpa_assemble_clouds[_rmat]: part_pcs [B, P, N, 3], valids [B, P] (a part is real iff its entry == 1), S predicted
 * poses rot [S, B, P, 4] (quaternions, real part first, not normalised) or [S, B, P, 9] (row-major matrices) with
 * trans [S, B, P, 3], the ground truth gt_rot [B, P, 4 | 9], gt_trans [B, P, 3], colors [C, 3]; all contiguous fp32.
 *   offsets int64 [B + 1]: shape b owns the rows offsets[b] : offsets[b + 1] of every slab, counted in points;
 *     offsets[b + 1] - offsets[b] = (valid parts of b) * N.
 *   clouds fp32 [S + 1, B * P * N, 6] is the capacity; only the first offsets[B] rows of a slab are written, no row
 *     behind them is touched.  Slab s < S holds prediction s, slab S the ground truth.  A row is (x, y, z, r, g, b):
 *     xyz exactly what mpa_pose_apply[_rmat]_forward writes for the point (same operations, same order, no FMA), the
 *     colour colors[k] with k the part's rank among the valid parts of its shape.  Parts in slot order, points in
 *     their order inside the part.
 * Two launches (the prefix over valids, then the posing), no host synchronisation, no atomics: capturable and
 * bit-identical from run to run.  Padded slots are never read: any values in their points and poses leave every
 * output bit unchanged.  Envelope: C >= P (refused otherwise), B * P < 2^31, N <= 65535 * 256.  B == 0 is a no-op;
 * with P == 0 or N == 0 only offsets (all zero) is written.  S == 0 writes the ground-truth slab alone.
 *
 * mpa_mesh_pose_parts: the triangles of M selected parts of a MeshStore (tri float64 [F, 9] = origin, e1, e2;
 * part_face_off int64 [parts_total + 1]) posed in one launch.  slot_part int64 [M]: a store part id, or < 0 for a
 * slot that owns no rows and touches nothing; out_face_off int64 [M + 1]: slot m writes the rows
 * out_face_off[m] : out_face_off[m + 1] (its part's face count; fewer rows truncate, rows >= faces_out are never
 * written); max_faces: the largest face count of a slot (sizes the grid).  gt_rmat / pred_rmat [M, 9] row-major and
 * gt_trans / pred_trans [M, 3] fp32.  Three outputs fp32 [faces_out, 3, 3], vertex triples per face:
 *   orig  v0 = origin, v1 = origin + e1, v2 = origin + e2
 *   input R_gt^T (v - T_gt)            (the part as the network sees it)
 *   pred  R_pred . input + T_pred
 * all in float64 on the fp32 poses widened -- (a b + c d) + e f per row, left to right, no FMA -- and rounded to
 * fp32 once at the store.
 * ---------------------------------------------------------------------------------------------- */
int mpa_assemble_clouds(const float* part_pcs, const float* valids, const float* quat, const float* trans,
                        const float* gt_quat, const float* gt_trans, const float* colors, int64_t S, int64_t B,
                        int64_t P, int64_t N, int64_t C, int64_t* offsets, float* clouds, void* stream);
int mpa_assemble_clouds_rmat(const float* part_pcs, const float* valids, const float* rmat, const float* trans,
                             const float* gt_rmat, const float* gt_trans, const float* colors, int64_t S, int64_t B,
                             int64_t P, int64_t N, int64_t C, int64_t* offsets, float* clouds, void* stream);
int mpa_mesh_pose_parts(const double* tri, const int64_t* part_face_off, int64_t parts_total, const int64_t* slot_part,
                        const int64_t* out_face_off, int64_t M, int64_t faces_out, int64_t max_faces,
                        const float* gt_rmat, const float* gt_trans, const float* pred_rmat, const float* pred_trans,
                        float* orig, float* input, float* pred, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Contact points of a batch (csrc/contact_points.hip) -- the table `calc_connectivity_acc` consumes
 * (multi_part_assembly/utils/eval_utils.py:56-99).  The reference only ever loads it from the PartNet release's
 * `contact_points/pairs_with_contact_points_*.npy` files (datasets/partnet_data.py:210-222); here it is computed from
 * what a batch carries, by an all-pairs closest-pair search between the posed parts.
 *
 * Inputs, contiguous fp32: part_pcs [B, P, N, 3] canonical; valids [B, P] (a part is real iff its entry == 1);
 * trans [B, P, 3]; rotations as quaternions [B, P, 4] (real part first, not normalised; Rotation3D's zero-quaternion
 * rule is applied: norm <= 0.5 -> identity, the test of mpa_quat_sanitize) or, for the _rmat twin, row-major matrices
 * [B, P, 3, 3]; thre_sq, a bound on the SQUARED distance.  Inputs are finite.
 * Arithmetic: posed_i[a] is the coordinate mpa_pose_apply[_rmat]_forward gives for point a of part i, bit for bit;
 * d(a, c) = (dx*dx + dy*dy) + dz*dz with every operation rounded -- the Chamfer contract above.
 * For every sample and every pair i < j of real parts, (a*, c*) is the lexicographically first minimiser of
 * d(posed_i[a], posed_j[c]) (lowest a, then lowest c) and dmin that minimum.
 *   contact_points [B, P, P, 4]: dmin < thre_sq: row [b, i, j] = (1, part_pcs[b, i, a*]) and row [b, j, i] =
 *     (1, part_pcs[b, j, c*]) -- CANONICAL coordinates, copied bit for bit (the metric poses them itself); otherwise both
 *     rows are zeros.  The diagonal and every row and column of a padded slot are zeros.
 *   min_dist [B, P, P] (NULL: skipped): symmetric, dmin of every real pair whatever the flag, 1e32 on the diagonal and
 *     in padded slots.
 *   index [B, P, P] int32 (NULL: skipped): [b, i, j] = a*, [b, j, i] = c*, -1 on the diagonal and in padded slots.
 * Every element of every output is written on every call.  Padded slots are never read: NaN in their points and poses
 * changes no output bit.  One launch, no atomics, a fixed reduction order, no host synchronisation, a launch
 * configuration that depends on the sizes only: capturable, bit-identical from run to run.  When neither min_dist nor
 * index is requested, a pair whose posed bounding boxes are at least thre_sq apart (the gap evaluated with the same
 * rounded formula, a lower bound of every computed d) is not searched; the outputs are those of the full search.
 * Envelope: 1 <= N <= 2048 (both posed parts live in LDS, 24 N bytes), 1 <= P <= 64, B >= 0, 4 * B * P * P < 2^31;
 * outside it the call is refused with MPA_EINVAL.  No workspace.
 * ---------------------------------------------------------------------------------------------- */
int mpa_contact_points(const float* part_pcs, const float* valids, const float* quat, const float* trans, float thre_sq,
                       int64_t B, int64_t P, int64_t N, float* contact_points, float* min_dist, int32_t* index,
                       void* stream);
int mpa_contact_points_rmat(const float* part_pcs, const float* valids, const float* rmat, const float* trans,
                            float thre_sq, int64_t B, int64_t P, int64_t N, float* contact_points, float* min_dist,
                            int32_t* index, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet++ sampling and grouping (csrc/pointnet2_ops.hip) -- the operators of the reference's CUDA-only extension
 * `pointnet2_ops` that its set-abstraction modules use (pointnet2_ops/pointnet2_utils.py: furthest_point_sample,
 * ball_query, grouping_operation, gather_operation; kernels in _ext-src/src/sampling_gpu.cu, ball_query_gpu.cu,
 * group_points_gpu.cu).  multi_part_assembly_amd/pointnet2_ref.py restates every definition below in numpy.
 * All arithmetic is IEEE fp32, one operation at a time in the written order, no fused multiply-add.  Inputs are
 * contiguous; indices are int32.  No call synchronises, every launch configuration depends on the sizes only
 * (capturable), every output element is written on every call, two calls give the same bits.
 *
 * mpa_furthest_point_sample: xyz [M, N, 3] -> idx [M, npoint].  idx[0] = 0; the running distance temp[k] of every point
 *   starts at 1e10.  Round j takes old = idx[j-1]; a point k with (double)((x*x + y*y) + z*z) <= 1e-3 is skipped (never
 *   updated, never chosen); every other point gets d = (dx*dx + dy*dy) + dz*dz against `old`, temp[k] = min(d, temp[k]),
 *   and idx[j] is the point of largest temp, 0 when every point is skipped.  Equal distances are decided as the
 *   reference's block reduction decides them under ITS block size T = min(512, 2^floor(log2 N)): the point whose
 *   reference thread k mod T, read with its log2 T bits reversed, is smallest; inside one thread the smallest k.
 *   npoint > N is legal (indices repeat).  Non-finite coordinates: unspecified indices inside [0, N), and the call
 *   terminates.  N <= 4096: no workspace (points and distances stay in registers and LDS); above, the distances live in
 *   the workspace, mpa_furthest_point_sample_workspace bytes, 256-byte aligned.  N >= 1 unless M or npoint is 0.
 * mpa_ball_query: xyz [M, N, 3], new_xyz [M, S, 3] -> idx [M, S, nsample]: the first nsample indices k, ascending, with
 *   (cx-x)^2 + (cy-y)^2 + (cz-z)^2 < radius * radius (fp32, strict; the sum left to right); the remaining slots repeat
 *   the first hit; a ball without a hit is all zeros.
 * mpa_group_points_forward: features [M, C, N], idx [M, S, K] -> out [M, C, S, K], out[m,c,j,l] = features[m,c,idx[m,j,l]].
 *   gather_operation is the call with K = 1.  An index outside [0, N) is never dereferenced: it reads as 0.
 * mpa_group_points_backward: grad_out [M, C, S, K] -> grad_features [M, C, N]: every element the fp32 sum of its
 *   contributions, added one after the other in ascending flat position j K + l, starting from 0; an index outside
 *   [0, N) contributes nothing.  No floating-point atomics.  Workspace: mpa_group_points_workspace bytes (the inverted
 *   index of every cloud), 256-byte aligned.
 * Sizes: every product of sizes that addresses a tensor (3 M N, M npoint, M S nsample, M C S K, M C N) stays below 2^31,
 * otherwise MPA_EINVAL.  Negative sizes and null pointers are refused before the device is touched; empty problems
 * return MPA_OK.
 * ---------------------------------------------------------------------------------------------- */
int mpa_furthest_point_sample_workspace(int64_t M, int64_t N, int64_t* bytes);
int mpa_furthest_point_sample(const float* xyz, int64_t M, int64_t N, int64_t npoint, void* workspace, int32_t* idx,
                              void* stream);
int mpa_ball_query(const float* xyz, const float* new_xyz, float radius, int64_t M, int64_t N, int64_t S,
                   int64_t nsample, int32_t* idx, void* stream);
int mpa_group_points_forward(const float* features, const int32_t* idx, int64_t M, int64_t C, int64_t N, int64_t S,
                             int64_t K, float* out, void* stream);
int mpa_group_points_workspace(int64_t M, int64_t N, int64_t S, int64_t K, int64_t* bytes);
int mpa_group_points_backward(const float* grad_out, const int32_t* idx, int64_t M, int64_t C, int64_t N, int64_t S,
                              int64_t K, void* workspace, float* grad_features, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet++ feature propagation (csrc/pointnet2_interp.hip) -- the remaining operators of `pointnet2_ops`
 * (pointnet2_ops/pointnet2_utils.py: three_nn, three_interpolate; kernels in _ext-src/src/interpolate_gpu.cu), which its
 * `PointnetFPModule` uses.  The rules of the block above hold: IEEE fp32, one operation at a time in the written order, no
 * fused multiply-add; contiguous inputs, int32 indices; no call synchronises, every launch configuration depends on the
 * sizes only (capturable), every output element is written on every call, two calls give the same bits, no floating-point
 * atomics.  multi_part_assembly_amd/pointnet2_ref.py restates every definition in numpy.
 *
 * mpa_three_nn: unknown [M, n, 3], known [M, m, 3] -> dist [M, n, 3], idx [M, n, 3].  For every unknown point the known
 *   points are walked in ascending k with d = ((ux-x)*(ux-x) + (uy-y)*(uy-y)) + (uz-z)*(uz-z); three running bests start
 *   at (+inf, index 0) and take d through the strict cascade: d < best1 shifts best1, best2 down and takes the first slot,
 *   else d < best2 shifts best2 down and takes the second, else d < best3 takes the third.  Equal distances therefore keep
 *   the lower index first, and a NaN d is never inserted.  dist holds the correctly rounded fp32 square roots of the three
 *   bests (the reference's wrapper takes them in a second launch), idx their indices; with m < 3 the unused slots stay
 *   (inf, 0).  m >= 1 and n >= 1 unless M is 0.
 * mpa_three_interpolate_forward: features [M, C, m], idx [M, n, 3], weight [M, n, 3] -> out [M, C, n],
 *   out[b,c,j] = (f1*w1 + f2*w2) + f3*w3 with fk = features[b,c,idx[b,j,k]]; an index outside [0, m) is never
 *   dereferenced: its fk reads as 0, the rule of mpa_group_points_forward.
 * mpa_three_interpolate_backward: grad_out [M, C, n] -> grad_features [M, C, m]: every element the fp32 sum, started at
 *   0, of the products grad_out[b,c,j] * weight[b,j,k] over the pairs (j, k) with idx[b,j,k] == i, added one after the
 *   other in ascending flat position 3 j + k; an index outside [0, m) contributes nothing.  Workspace:
 *   mpa_three_interpolate_workspace bytes (the inverted index of every cloud: mpa_group_points_backward's, over 3 n
 *   positions), 256-byte aligned.
 * Sizes: 3 M n, 3 M m, M C n and M C m stay below 2^31, otherwise MPA_EINVAL.  Negative sizes and null pointers are refused
 * before the device is touched; empty problems return MPA_OK.
 * ---------------------------------------------------------------------------------------------- */
int mpa_three_nn(const float* unknown, const float* known, int64_t M, int64_t n, int64_t m, float* dist, int32_t* idx,
                 void* stream);
int mpa_three_interpolate_forward(const float* features, const int32_t* idx, const float* weight, int64_t M, int64_t C,
                                  int64_t m, int64_t n, float* out, void* stream);
int mpa_three_interpolate_workspace(int64_t M, int64_t n, int64_t m, int64_t* bytes);
int mpa_three_interpolate_backward(const float* grad_out, const int32_t* idx, const float* weight, int64_t M, int64_t C,
                                   int64_t n, int64_t m, void* workspace, float* grad_features, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet++ set-abstraction level for evaluation (csrc/pointnet2_sa_mlp.hip): gather, three (GEMM, per-channel scale and
 * shift, ReLU) layers, max over the samples of every centre, in one kernel -- the shared MLP of a `PointnetSAModule` whose
 * BatchNorms are in eval() mode, without the [M, C, S, K] tensors.  `sa_mlp_max` of multi_part_assembly_amd/pointnet2_ref.py
 * restates it in numpy.
 *
 * mpa_sa_mlp_pack: one layer, W [Cout, Cin] fp32 and gamma, beta, running_mean, running_var [Cout], into `packed`
 *   (mpa_sa_mlp_packed_bytes bytes = 6 Cout Cinp + 8 Cout with Cinp = Cin rounded up to the k-chunk of 32; 16-byte aligned):
 *     bf16 [Cinp / 32][Cout][3][32]   the planes h, m, l of W[n, 32 c .. 32 c + 31] (the split of csrc/dg_gemm_split.h:
 *                                     h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); h + m + l == x), zeros past Cin
 *     fp32 [Cout]                     scale = gamma / sqrt(running_var + eps)     (IEEE fp32 division and square root)
 *     fp32 [Cout]                     shift = beta - running_mean * scale         (no fused multiply-add)
 *   One launch, every byte of the buffer written.  Cout a multiple of 32 in [32, 512], Cin in [1, 515]; Cout = 0: MPA_OK.
 * mpa_sa_mlp_max_forward: xyz [M, N, 3], new_xyz [M, S, 3], features [M, N, C] (POINT-major; NULL exactly when C = 0),
 *   idx [M, S, K], three packed layers of widths (3 + C -> C1), (C1 -> C2), (C2 -> C3)  ->  out [M, S, C3], point-major.
 *   Row (m, j, l) of the virtual input is [xyz[m, idx[m,j,l]] - new_xyz[m, j] ; features[m, idx[m,j,l]]], the subtraction in
 *   fp32 before any product.  An index outside [0, N) is never dereferenced: it reads a zero point and zero features (the
 *   centre is still subtracted), the rule of mpa_group_points_forward.  new_xyz == NULL and idx == NULL together (the
 *   reference's GroupAll) need S = 1, K = N: the row is [xyz[m, l] ; features[m, l]].
 *   a_l = relu(scale_l * (W_l a_{l-1}) + shift_l) for l = 1, 2, 3 and out[m, j, :] = max over l of a_3.  Products: the
 *   fp32-grade six-term split-bf16 form on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the summation order is
 *   unspecified.  No activation goes to global memory.
 *   Envelope: C1, C2, C3 multiples of 32 in [32, 512], 0 <= C <= 512, K >= 1, N >= 1; outside it MPA_EINVAL with a message
 *   that names the offending size.  3 M N, 3 M S, M N C, M S K and M S C3 stay below 2^31.  Contiguous inputs; no call
 *   synchronises; the launch configuration depends on the sizes only (capturable); every output element is written on
 *   every call; two calls give the same bits; negative sizes and null pointers are refused before the device is touched;
 *   M, S or C3 = 0 returns MPA_OK; non-finite inputs give unspecified values and no fault.
 * ---------------------------------------------------------------------------------------------- */
int mpa_sa_mlp_packed_bytes(int64_t Cout, int64_t Cin, int64_t* bytes);
int mpa_sa_mlp_pack(const float* W, const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, float eps, int64_t Cout, int64_t Cin, void* packed, void* stream);
int mpa_sa_mlp_max_forward(const float* xyz, const float* new_xyz, const float* features, const int32_t* idx, int64_t M,
                           int64_t N, int64_t S, int64_t K, int64_t C, const void* layer1, const void* layer2,
                           const void* layer3, int64_t C1, int64_t C2, int64_t C3, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Repulsion loss (csrc/repulsion.hip) -- `repulsion_cd_loss` of the reference (multi_part_assembly/utils/loss.py:205-225):
 * the Chamfer distance of every pair of parts of a shape, hinged at `thre`, without the two [B P P, N, 3] expansions.
 * multi_part_assembly_amd/repulsion_ref.py restates every definition below in numpy, in float32 and float64.
 *
 * Inputs, contiguous fp32: part_pcs [B, P, N, 3], the POSED clouds (the operator is the same for every rotation form);
 * valids [B, P] (a part is valid iff its entry == 1); thre by value.  Valid parts hold finite coordinates; padded slots are
 * never read (NaN there changes no output bit).  With nv the number of valid parts of sample b:
 *   loss_b = [nv thre + 2 sum_{i<j, both valid} max(0, thre - cd_ij)] / nv^2,    cd_ij = mean_n d1[n] + mean_m d2[m],
 *   d1[n] = min_m d(a_n, b_m), d2[m] = min_n d(a_n, b_m) over the points a of part i and b of part j, with the Chamfer
 *   contract above: d = (dx*dx + dy*dy) + dz*dz, every operation rounded, strict `<` in index order, (1e32, -1) for a point
 *   that never sees d < 1e32 -- d1, d2 and both index lists are those of mpa_chamfer_forward for the pair, bit for bit.
 *   (The reference sums all P x P pairs: every unordered pair twice, and `thre` per valid part for the diagonal, whose cd
 *   is 0.)  A mean is `ordered_sum` / N: 256 partial sums over the points t, t + 256, ... in ascending order, six butterfly
 *   steps p[t] += p[t ^ off] (off = 32 ... 1) in every group of 64, the four groups left to right.  The hinges are added in
 *   slot order (i ascending, then j), started at 0.  nv = 0 gives NaN (0 / 0), as the reference does.
 * Outputs: loss [B]; cd [B, P, P] (NULL: skipped) symmetric, 0 on the diagonal and for a pair with a padded member; dists
 * [B, P (P - 1) / 2, 2, N] (NULL: skipped; a diagnostic) d1 and d2 of every searched pair, other rows unwritten.
 * The prune: when cd is not requested, a pair whose bounding boxes are at least `thre` apart -- the gap g evaluated with
 * the rounded formula of mpa_contact_points, a lower bound of every computed d -- is not searched.  Then each mean is at
 * least g (1 - N 2^-24) and cd >= 2 g (1 - N 2^-24) >= thre, the hinge is exactly zero: the prune never changes loss or
 * gradient.
 * Workspace: mpa_repulsion_cd_workspace bytes, 256-byte aligned, written by the forward and read by the backward: per pair
 * slot a flag byte (0 not searched: padded member or pruned; 1 searched, thre - cd < 0; 2 hinged, thre - cd >= 0 -- the
 * rule of torch's clamp_min) at flag_offset, and for every searched pair the two 16-bit arg-min lists [B, slots, N] at
 * idx1_offset (points of i -> part j) and idx2_offset (points of j -> part i), 0xffff for -1; the lists of other pairs
 * are unwritten.  The offset pointers may be NULL.
 * Backward: grad_loss [B] -> grad_pcs [B, P, N, 3], every element written.  c_b = (-grad_loss[b] * 2) / ((nv * nv) * N).
 * Point n of part i takes, over its hinged partners j in ascending order, first c_b * (2 (a_n - b_{idx[n]})) for its own
 * minimum and then c_b * (2 (a_n - b_m)) for every point m of j whose minimum lands on it, in ascending m; every product
 * and sum rounded, per coordinate, no floating-point atomics.  Padded slots, pairs that are not hinged and a sample
 * without a valid part get exact zeros (the reference's gradient of such a sample is NaN).
 * Forward: two launches (one block per pair slot, one per sample); backward: one (one block per part).  No atomics, no
 * host synchronisation, launch configurations that depend on the sizes only: capturable, bit-identical from run to run.
 * Envelope: 1 <= N <= 2048 (both parts live in LDS, 24 N bytes), 1 <= P <= 64, B >= 0, B P P N < 2^31; outside it
 * MPA_EINVAL.  Negative sizes and null pointers are refused before the device is touched; B = 0 returns MPA_OK.
 * ---------------------------------------------------------------------------------------------- */
int mpa_repulsion_cd_workspace(int64_t B, int64_t P, int64_t N, int64_t* bytes, int64_t* flag_offset, int64_t* idx1_offset,
                               int64_t* idx2_offset);
int mpa_repulsion_cd_forward(const float* part_pcs, const float* valids, float thre, int64_t B, int64_t P, int64_t N,
                             void* workspace, float* loss, float* cd, float* dists, void* stream);
int mpa_repulsion_cd_backward(const float* grad_loss, const float* part_pcs, const float* valids, int64_t B, int64_t P,
                              int64_t N, const void* workspace, float* grad_pcs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPA_HIP_H_ */
