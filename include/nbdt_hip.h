/*
 * nbdt_hip.h -- C-ABI of libnbdt_hip.so, the MI355X (gfx950) native hot path of
 * Neural-Backed Decision Trees.
 *
 * The reference (alvinwan/neural-backed-decision-trees) is 100% Python and has no
 * FFI/plugin registry: its boundary for this path is the nn.Module API
 *   nbdt/model.py:65-273   EmbeddedDecisionRules / Hard* / Soft*   (rules layer)
 *   nbdt/loss.py:97-266    TreeSupLoss / SoftTreeSupLoss           (tree-supervision loss)
 *   nbdt/models/resnet.py:42-149, nbdt/models/wideresnet.py:1-40   (backbones; every op a
 *                          stock aten/cuDNN kernel: Conv2d, BatchNorm2d, ReLU, avg-pool, Linear)
 *   main.py:207,233-239    SGD(momentum .9, wd 5e-4) train step
 * Each entry point below replaces the stock-op sequence named in its comment.  The host side
 * (neural-backed-decision-trees_amd/nbdt, Python, same class names/signatures as the
 * reference) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer borrowed for the duration
 *     of the stream-ordered call unless marked "host"; the caller (PyTorch caching allocator)
 *     owns all tensors.  The library owns only tree handles.
 *   - every call returns 0 on success, a negative NBDT_E* code on failure and never throws;
 *     nbdt_last_error() returns a thread-local message for the last failure.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous and re-entrant across streams/devices.
 *   - activations are "padded NHWC bf16": [B][H+2][W+2][C] with a zero one-pixel border
 *     (so every 3x3 tap is in-bounds); kernels write interiors only.
 *   - conv weights are [Cout][taps][Cin] bf16 ("KRSC"), fp32 masters in the same order.
 *
 * Size limits (nbdt_version() >= 130; DESIGN.md section 26 has the derivation of each).  A tensor at or past its limit is
 * refused with NBDT_EINVAL before any HIP call -- nothing is truncated and no wrapped address is formed.  "Elements" are
 * elements of the tensor's type; most kernels keep signed 32-bit element offsets from the tensor's base:
 *   nbdt_conv_igemm[_stats|_affine|_bnbwd|_multi], nbdt_conv_plan
 *                          output (= residual, accumulate, bn_x) elements B*out_bs + out_base < 2^31; input elements
 *                          B*in_bs + in_base + max tap_off < 2^31; weight elements cout*w_ntaps*cin < 2^31; pixels
 *                          B*gh*gw < 2^31
 *   nbdt_conv_wgrad        B*x_bs + x_base + max tap_off < 2^31, B*g_bs + g_base < 2^31, cout*w_ntaps*cin < 2^31, pixels < 2^31
 *   nbdt_conv_pw           B*in_bs + tap_off < 2^31, B*out_bs < 2^31, cin*cout < 2^31, pixels < 2^31
 *   nbdt_conv_seg_create   input bytes B*(gh+2)*(gw+2)*pix_stride*2 < 2^32; per class B*out_bs + out_base < 2^31; pixels < 2^31
 *   nbdt_conv_group_*      padded pixels B*(H+2)*(W+2) < 2^31 (no limit on elements: 64-bit addresses)
 *   nbdt_bn_*, nbdt_pool_bn_bwd_*, nbdt_bn_act_*, nbdt_dwconv_*
 *                          padded elements B*(H+2)*(W+2)*C < 2^31 (the depthwise entries: of the input-side tensor);
 *                          nbdt_bn_apply_s2d also B*(H/2+2)*(W/2+2)*4C < 2^31 for its output
 *   nbdt_stem_wgrad        output pixels B*Ho*Wo < 2^31 - 2^22;  nbdt_stem_conv_pad / nbdt_stem_wgrad_pad: < 2^25
 *   nbdt_seg_*             blocks N*ceil(HW/64) < 2^31; nbdt_seg_soft_tree_loss and nbdt_seg_stats_accumulate also pixels
 *                          N*HW < 2^31 (the loss counts the valid pixels, the statistics count per block, in 32 bits)
 *   nbdt_upsampled_xent    pixels N*H*W < 2^31 (one forward block per 64 of them); H, W <= 2^22 (the source index is an
 *                          fp32: dst + 0.5f stays exact); C <= 262,140 (class chunks in grid.y); no limit on N*C*h*w
 *                          (64-bit offsets)
 *   no limit below the launch grid (64-bit offsets throughout): nbdt_stem_conv, nbdt_stem_patches, nbdt_maxpool3x3s2_*,
 *   nbdt_dropout_*, nbdt_linear_*, nbdt_se_*, nbdt_mix_batch, nbdt_augment_batch*, nbdt_policy_*batch*,
 *   nbdt_resized_crop_*batch* (datasets and batches past 4 GiB are fine; one image has H, W <= 4096),
 *   nbdt_group_logits[_backward], nbdt_superclass_accumulate (grid-stride loops over the batch).
 */
#ifndef NBDT_HIP_H
#define NBDT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBDT_OK 0
#define NBDT_EINVAL (-1)   /* bad argument / unsupported shape */
#define NBDT_EHIP (-2)     /* HIP runtime error */
#define NBDT_ENOMEM (-3)

/* element types of the logits handed to the rules layer */
#define NBDT_F32 0
#define NBDT_BF16 1
#define NBDT_F16 2

const char* nbdt_last_error(void);
/* Name of the device kernel the calling thread's last nbdt_conv_igemm* call launched ("conv3x3_pp_kernel",
 * "conv3x3_halo_kernel", "conv_igemm_dma_kernel"): lets the parity tests assert WHICH kernel they exercised. */
const char* nbdt_debug_last_igemm(void);
/* the same with the kernel's template arguments, spelled as rocprofv3 prints it ("conv3x3_pp_kernel<5, false, 0, 8, false,
 * 2>"): what bench.py compares with the kernel names of a committed PMC traffic file before quoting it */
const char* nbdt_debug_last_igemm_full(void);
const char* nbdt_debug_last_wgrad(void);      /* same for nbdt_conv_wgrad */
/* Which form the calling thread's last rules launch took (nbdt_soft_forward, nbdt_soft_backward, the tree losses,
 * nbdt_hard_forward, nbdt_node_outputs, nbdt_tree_stats_accumulate): "lds" (rows and staged operands in LDS),
 * "lds-unstaged" (rows in LDS, direct-indexed chains), "global" (rows in global memory), "pixel" (the nbdt_seg_*
 * entries: one lane per pixel of an NCHW tensor, nbdt_version() >= 129; nbdt_seg_stats_accumulate among them,
 * nbdt_version() >= 132), "" before the first launch.
 * See "Size limits" at nbdt_tree_create.  nbdt_version() >= 127. */
const char* nbdt_debug_last_rules_path(void);
/* Form of the per-sample rules kernels (process-wide, default 0; nbdt_version() >= 127).  0: automatic -- the LDS forms
 * wherever a sample's row fits LDS, exactly as before this switch existed, and the global-row form only where they
 * cannot run.  1: the global-row form for every hierarchy; for tests and measurements (it is slower wherever the LDS
 * forms run).  The diagnostics and the fused head have no global-row form and ignore the switch.  Anything else is
 * NBDT_EINVAL. */
int nbdt_set_rules_path(int mode);
int nbdt_get_rules_path(void);
int nbdt_version(void);
/* Deterministic mode (process-wide switch, default off).  The reference's CPU path (stock ATen ops,
 * nbdt/models/resnet.py:69-74) gives the same bits on every run; the fast path does not: every cross-block fp32
 * reduction of the backbone -- the 32 replicated BatchNorm accumulators (nbdt_bn_stats, nbdt_bn_bwd_reduce[_cus],
 * nbdt_pool_bn_bwd_reduce), the split-K weight gradients (nbdt_conv_wgrad, nbdt_stem_wgrad, nbdt_linear_bwd) and the
 * per-tile statistics of the conv epilogues (nbdt_conv_igemm_stats, nbdt_conv_igemm_bnbwd) -- goes through fp32
 * atomics whose order changes from run to run, and a 1-ulp difference in a BatchNorm sum moves bf16 roundings and
 * ReLU masks downstream (two runs of one WRN-28-10 step differ by ~0.17 relative L2 in the gradient).  With the switch
 * on, each of those reductions adds into a zeroed, library-owned row per block / per pixel split (one add per address)
 * and a fold kernel sums the rows in index order: two runs of the same launches on the same inputs are then
 * bit-identical, whatever streams they were issued on.  Slower (an extra fold per reduction, 64+ MB of workspace per
 * (device, stream), allocated with hipMalloc on first use -- not capturable in a hipGraph); the arithmetic differs
 * from the default mode only in summation order.  Scope: every kernel of the three backbones -- the EfficientNet-
 * specific reductions too (nbdt_dwconv_fwd's statistics, nbdt_dwconv_bwd_weight, nbdt_bn_act_pool, nbdt_bn_act_bwd,
 * nbdt_se_gate_bwd's parameter gradients) -- and the rules layer, whose only atomics add integers
 * (nbdt_tree_stats_accumulate) and give the same sums in any order. */
int nbdt_set_deterministic(int32_t on);
int nbdt_get_deterministic(void);
/* Epilogue of the K-split weight-gradient kernel (nbdt_conv_wgrad on the 3x3 stride-1 shapes; process-wide, default 1).
 * 1: each (pixel split, tile) block writes its partial sums with plain stores into that split's copy of dw in the
 *    per-(device, stream) workspace (the one deterministic mode uses, same hipGraph rule: one eager launch first) and
 *    a streaming pass adds the copies to dw in split order: the sum no longer depends on block timing.  The L2 retires
 *    fp32 atomics at ~1.2 TB/s whatever their shape: alone the launch is 4-8 % faster on the WRN-28-10 shapes and 20-27 %
 *    on ResNet18's at batch 128 (fold included); training steps: WRN-28-10 unchanged, ResNet18 1-4 % faster
 *    (profiles/r05_wgrad_store_epilogue_ab.txt).  Launches with more than 64 pixel splits keep the atomics, and so do
 *    CU-budgeted launches (desc.cu_budget > 0: an HBM-bound pass runs beside them, the fold would compete with it).
 * 0: fp32 atomics into dw (rounds 3-4).  Deterministic mode always takes the stores for that kernel. */
int nbdt_set_wgrad_store_epilogue(int32_t on);
int nbdt_get_wgrad_store_epilogue(void);
/* CUs (0..128, process-wide, default 0) the one-block-per-CU MFMA kernels leave free: the persistent forward / data-
 * gradient kernel launches 8 x (32 - ceil(n / 8)) blocks instead of 256 and the weight gradient is sized for at most
 * 256 - n.  For data-parallel training: RCCL's all-reduce kernels (one block per channel, NCCL_MAX_NCHANNELS of them)
 * run beside the backward pass, and a persistent block that finds its CU held by one of them starts when that block
 * ends -- the whole launch then waits for it (measured with a look-alike holder kernel: up to +1.7 ms per step).  The
 * engine sets n = the channel count while gradient buckets are in flight and 0 otherwise.  Results do not change
 * (same tiles, other block -> tile assignment).  Replaces nothing in the reference (DataParallel, main.py:160-162). */
int nbdt_set_reserved_cus(int32_t n);
int nbdt_get_reserved_cus(void);
/* Nontemporal-load threshold of the streaming BatchNorm passes (process-wide, default 96 MiB = 100663296 bytes;
 * nbdt_version() >= 109).  nbdt_bn_apply, nbdt_bn_bwd_apply_cus, nbdt_bn_bwd_reduce_cus and nbdt_bn_bwd_cus read their
 * operands with nontemporal loads when the padded tensor, B * (H+2) * (W+2) * C * 2 bytes, is at least this many bytes,
 * and with plain loads otherwise.  The two forms compute the same bits; only what the caches keep differs.  Must be
 * >= 0; 0 makes every launch nontemporal.  nbdt_debug_last_stream_nt: what the calling thread's last launch of those
 * four chose (1 nontemporal, 0 plain, -1 none yet) -- for tests that must know which instantiation they ran. */
int nbdt_set_stream_nt_min_bytes(int64_t bytes);
int64_t nbdt_get_stream_nt_min_bytes(void);
int nbdt_debug_last_stream_nt(void);
/* number of visible HIP devices (0 => the product path must refuse to run) */
int nbdt_device_count(void);

/* DMA-ordered weight tiles for the dense 3x3 kernel.  For every listed matrix W[rows][9][k] (bf16, rows % 32 == 0,
 * k % 32 == 0; the forward weights, or the transposed tap-reversed data-gradient copy) write tiles
 * [row block of 32*nt][k slice of 32][tap] of (32*nt) x 32 elements, each stored exactly as the kernel's LDS image
 * (row-major 64-byte rows with the 16-byte chunk index XOR (row>>2)&3), so that one 1-KiB LDS-DMA instruction reads
 * one contiguous KiB instead of sixteen 64-byte fragments 2.8 KB apart.  nt = 5 | 4 | 2 | 1 is the largest of these
 * dividing rows/32 (the kernel's cout tile).  table (device, int64 [n][5]): {src element offset, dst element offset,
 * rows, k, first tile index}; total_tiles = sum of (rows/(32*nt)) * (k/32) * 9. */
int nbdt_weight_tile_batched(const void* src_bf16, const int64_t* table, int32_t n, int64_t total_tiles,
                             void* dst_bf16, void* stream);

/* ------------------------------------------------------------------ hierarchy handle
 * Flattened form of nbdt/tree.py Tree/Node (build_class_mappings :105-125):
 *   N inner nodes in `tree.inodes` order (sorted wnid), node n owns child slots
 *   [node_off[n], node_off[n+1]);  slot s averages the logits of classes
 *   slot_cls[slot_off[s] .. slot_off[s+1]) (ascending);  class c lies under slots
 *   cls_slot[cls_off[c] .. cls_off[c+1]) (inode order: strictly ascending slot index, checked);  slot_next[s] = inode index of the
 *   child if it is an inner node, else -(class_index)-1.   All arrays are HOST pointers and are
 *   copied to `device`, together with the order in which a sample's lanes take the slots (longest first, dealt to
 *   the waves by load: csrc/rules.hip build_slot_schedule).
 * Size limits of the rules kernels: none for the rules and the losses (nbdt_soft_forward, nbdt_soft_backward,
 *   nbdt_soft_tree_loss[_ex], nbdt_hard_tree_loss[_ex], nbdt_hard_forward, nbdt_node_outputs,
 *   nbdt_node_logits_backward).  They take one of three forms, chosen per launch from the hierarchy alone:
 *   - the per-sample rows (2-3 floats per class and per child slot) plus the offset arrays fit 160 KB of LDS, and so
 *     does the sum of the leaf depths L = slot_off[R]: the kernels stage the gathered operands in LDS (ImageNet-1000:
 *     L = 11012);
 *   - the rows fit but L does not: they index through the maps directly -- same results, slower;
 *   - the rows do not fit (from roughly 2,300 classes of a binary hierarchy): the rows live in global memory, in the
 *     library's per-(device, stream) workspace: one row of about 3C + 2R floats per block of a grid of at most one
 *     block per CU, whatever the batch (0.6 MB per row at 21,841 classes; the workspace allocates at least 64 MB and
 *     25 % headroom: 187 MB there on 256 CUs).  NBDT_ENOMEM when the workspace cannot be
 *     allocated; under hipGraph capture the workspace's rule holds (one eager launch first).  Same arithmetic contract:
 *     node logits, node predictions, hard predictions and decision nodes / children are bit-equal to the LDS forms;
 *     inner nodes with more than 64 children have their softmax sums folded by the whole block, in a fixed order.
 *   Still limited (NBDT_EINVAL "hierarchy too large for LDS ..." / "classifier too wide for the fused head ..."):
 *   nbdt_tree_stats_accumulate keeps its rows and counters in LDS, and nbdt_head_soft_tree_loss takes at most 512
 *   classes and child slots. */
typedef struct nbdt_tree nbdt_tree;
int nbdt_tree_create(int device, int num_classes, int num_inodes, int root,
                     const int32_t* node_off, const int32_t* slot_off, const int32_t* slot_cls,
                     const int32_t* cls_off, const int32_t* cls_slot, const int32_t* slot_next,
                     nbdt_tree** out);
int nbdt_tree_destroy(nbdt_tree* t);
int nbdt_tree_max_depth(const nbdt_tree* t);

/* ------------------------------------------------------------------ rules layer
 * z: [B, C] logits, row stride ldz elements, element type ztype.  Outputs are fp32/int64,
 * dense row-major. */

/* SoftEmbeddedDecisionRules.forward (nbdt/model.py:207-242, 268-273): P[B,C] path probabilities */
int nbdt_soft_forward(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                      float* P, void* stream);
/* autograd of the above: gz[B,C] (fp32) = d<gP,P>/dz ; recomputes the forward from z */
int nbdt_soft_backward(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                       const float* gP, float* gz, void* stream);
/* SoftTreeSupLoss.forward + backward fused (nbdt/loss.py:191-203, 260-266) for
 * criterion = nn.CrossEntropyLoss():  loss = w_x*CE(z,y) + w_t*CE(P,y) (mean over B),
 * gz = grad_scale * dloss/dz.  row_loss: [B] fp32 scratch; loss: 1 fp32. */
int nbdt_soft_tree_loss(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                        const int64_t* y, float w_xent, float w_tree, float grad_scale,
                        float* row_loss, float* loss, float* gz, void* stream);
/* N1 -- classifier head + SoftTreeSupLoss forward AND backward in one launch: the logits never touch HBM.
 * Replaces nn.Linear (reference nbdt/models/resnet.py:126,148; pytorchcv `output`), TreeSupLoss.forward with the soft
 * rules (nbdt/loss.py:191-203, 264-266; nbdt/model.py:94-99, 207-242) and the Linear's autograd, i.e. the sequence
 * nbdt_linear_fwd -> nbdt_soft_tree_loss -> nbdt_linear_bwd, for classifiers of at most 512 classes / child slots
 * (NBDT_EINVAL beyond: use that sequence).
 *   pooled [B][K] fp32 features, W [C][K], bias [C] (nullable) fp32;  z = pooled W^T + bias (one wave per class,
 *   lanes over K, fused multiply-adds + xor butterfly: bit-identical to nbdt_linear_fwd for C < 64);
 *   loss / row_loss as nbdt_soft_tree_loss;  z_out [B][C] (nullable) = the logits the loss was computed on;
 *   gpooled [B][K] (nullable) = dL/dpooled;  gW [C][K], gb [C] (nullable) ACCUMULATE dL/dW, dL/db (+=). */
int nbdt_head_soft_tree_loss(const nbdt_tree* t, const float* pooled, const float* W, const float* bias, int64_t B,
                             int32_t K, const int64_t* y, float w_xent, float w_tree, float grad_scale,
                             float* row_loss, float* loss, float* z_out, float* gpooled, float* gW, float* gb,
                             void* stream);

/* HardTreeSupLoss.forward + backward fused (nbdt/loss.py:191-203, 212-257; label filtering
 * nbdt/model.py:127-143) for criterion = nn.CrossEntropyLoss():
 *   loss = mean_b[ w_xent*CE(z_b,y_b) + w_node * sum_{inner nodes n with y_b under n}
 *                                                   CE(node_logits(z_b, n), child_of(n, y_b)) ]
 * the caller folds the reference's weights into w_node = tree_weight * tsw * 2 / N (every pooled
 * (sample,node) row weighs tsw/(B*N/2), then TreeSupLoss.forward applies the schedule).
 * gz = grad_scale * dloss/dz.  row_loss: [B] fp32 scratch; loss: 1 fp32. */
int nbdt_hard_tree_loss(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                        const int64_t* y, float w_xent, float w_node, float grad_scale,
                        float* row_loss, float* loss, float* gz, void* stream);
/* ---- soft targets and label smoothing (nbdt_version() >= 116): the same two kernels for
 * criterion = nn.CrossEntropyLoss(label_smoothing = smoothing), 0 <= smoothing < 1, and -- the soft loss only -- for
 * probability targets [B, C], which is what MixUp / CutMix and soft-label transforms hand to a loss.
 *
 * nbdt_soft_tree_loss_ex.  Exactly one of y (int64 [B]) and tprob (fp32, row b at tprob + b*ldt, ldt >= C) is non-NULL.
 * With t the target row (onehot(y) for class indices) and eps = smoothing:
 *   t'_c = (1 - eps)*t_c + eps/C,   T = sum_c t'_c      (T is NOT assumed to be 1: torch does not normalise the row)
 *   row  = w_xent*(T*lse(z) - sum_c t'_c z_c) + w_tree*(T*lse(P) - sum_c t'_c P_c),   loss = mean of row over B
 *   gz   = grad_scale * dloss/dz: the direct term w_xent*(T*softmax(z) - t')/B plus w_tree*(T*softmax(P) - t')/B carried
 *          through the path products, as in nbdt_soft_tree_loss.
 * A class index outside [0, C) still gives a NaN loss; a dense row is used as given.  nbdt_soft_tree_loss is this entry
 * with tprob = NULL and smoothing = 0 (its kernel instantiation and bits are unchanged).
 *
 * nbdt_hard_tree_loss_ex.  Class-index targets only.  Every node term becomes, with K_n children and the label under
 * child s,  lse(s_n) - (1 - eps)*s_{n,s} - (eps/K_n)*sum_k s_{n,k}  (the criterion applied to the node's K_n logits); the
 * cross-entropy term is smoothed with eps/C.  nbdt_hard_tree_loss is this entry with smoothing = 0. */
int nbdt_soft_tree_loss_ex(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz, const int64_t* y,
                           const float* tprob, int64_t ldt, float smoothing, float w_xent, float w_tree,
                           float grad_scale, float* row_loss, float* loss, float* gz, void* stream);
int nbdt_hard_tree_loss_ex(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz, const int64_t* y,
                           float smoothing, float w_xent, float w_node, float grad_scale, float* row_loss, float* loss,
                           float* gz, void* stream);
/* VJP of get_node_logits over every inner node (nbdt/model.py:83-99): gs [B,R] fp32 gradient of
 * the child logits (slot-major, as written by nbdt_node_outputs) -> gz [B,C] fp32. */
int nbdt_node_logits_backward(const nbdt_tree* t, const float* gs, int64_t B, float* gz, void* stream);
/* HardEmbeddedDecisionRules.forward_with_decisions (nbdt/model.py:145-199): pred[B] int64,
 * optional onehot[B,C] fp32 (predicted_to_logits), optional decision buffers
 * [B, max_depth]: inode index / chosen child / its prob / node entropy (-1 padded). */
int nbdt_hard_forward(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                      int64_t* pred, float* onehot, int32_t* path_node, int32_t* path_child,
                      float* path_prob, float* path_entropy, void* stream);
/* EmbeddedDecisionRules.forward_nodes (nbdt/model.py:101-123): per-slot logits/probs [B,R],
 * per-node preds [B,N] int64 and entropy [B,N]; any output may be NULL. */
int nbdt_node_outputs(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                      float* logits, float* probs, int64_t* preds, float* entropy, void* stream);

/* Tree diagnostics of one evaluation batch in ONE launch (nbdt_version() >= 112): what the reference's ConfusionMatrix,
 * Entropy, TopDifference and NBDTEntropyMaxMin analyzers compute on the host (nbdt/analysis.py:133-180, 324-427), plus
 * per-node statistics it does not have.  The logits are read once and the node logits formed once; the per-node
 * softmax, the hard walk and the soft path product all work on them in LDS.
 *   y [B] int64 labels (required when any counter is requested).  A label outside [0, C) makes the sample count
 *   NOWHERE (the device-resident datasets hand out -1 for an out-of-range index row).
 *   stats (host pointer, nullable) holds device pointers; each may be NULL = not wanted.  Every counter is int64 and
 *   is ADDED TO, never overwritten: the caller zeroes once per pass and may split the pass into batches any way it
 *   likes -- all sums are integer sums, so the result is bit-identical whatever the split or the order of the atomics.
 *     totals[4]            samples with a valid label, backbone top-1 hits, hard-rules hits, soft-rules hits
 *     confusion_net / _hard / _soft [C*C]   entry [label * C + prediction]; predictions = argmax of z, the hard
 *                          walk's leaf, argmax of the soft path product; the first maximum wins everywhere
 *     node_counts[N*5]     per inner node (tree.inodes order), five counters side by side:
 *                          on_path (the label lies under the node), on_path_right (on_path and the node's argmax child
 *                          contains the label), visited (the hard walk passes the node), visited_on_path,
 *                          visited_on_path_right.  "Contains the label" is membership in the child's leaf set: in a
 *                          single-parent hierarchy the reference's class_index_to_child_index[y][0]; in the multi-parent
 *                          WordNet graphs ANY child that holds the class counts.
 *     node_entropy[N*2]    per inner node, over the valid samples: sum of the node's entropy (the Categorical entropy
 *                          nbdt_node_outputs reports) and sum of its square, each fp32 value rounded to the nearest
 *                          multiple of 2^-32 and added as an integer (divide by 2^32 to read it)
 *     first_error_depth[max_depth + 1]   index d: samples whose hard walk first picks a child that does not contain
 *                          the label at depth d (root = 0); index max_depth: samples that never leave the path
 *   scores (nullable) fp32 [B,3], WRITTEN: entropy of softmax(z) (Entropy.score), top-1 minus top-2 softmax
 *   probability (TopDifference.score), max minus min of the entropies along the hard walk with the reference's
 *   leading 0 of the root entry included (NBDTEntropyMaxMin.score).
 * Limits: the LDS forms' (the sample rows and the offset arrays in 160 KB of LDS: there is no global-row form of the
 * diagnostics, whose confusion matrices alone are C*C int64), plus 28 bytes of LDS per inner node for the block's
 * counters.  NBDT_EINVAL "hierarchy too large for LDS: ..." beyond them. */
typedef struct nbdt_tree_stats {
  int64_t* totals;
  int64_t* confusion_net;
  int64_t* confusion_hard;
  int64_t* confusion_soft;
  int64_t* node_counts;
  int64_t* node_entropy;
  int64_t* first_error_depth;
} nbdt_tree_stats;
int nbdt_tree_stats_accumulate(const nbdt_tree* t, const void* z, int ztype, int64_t B, int64_t ldz,
                               const int64_t* y, const nbdt_tree_stats* stats, float* scores, void* stream);

/* ---- the rules on NCHW logits, one lane per pixel (nbdt_version() >= 129; csrc/rules_pixel.h): SegNBDT, HardSegNBDT,
 * SoftSegNBDT (nbdt/model.py:376-399) and SoftSegTreeSupLoss (nbdt/loss.py:318-327) without the reference's permutes
 * to [N*H*W, C] rows and back.
 *   z: [N, C, HW] logits of type ztype; the HW pixels of a plane are contiguous, image n / channel c starts at element
 *   n*zi + c*zc (int64 element strides, so a channel-sliced view works; zc >= HW, zi >= (C-1)*zc + HW).  Every offset is
 *   64-bit.  Outputs are dense fp32 / int64 in the same [N, C, HW] / [N, HW] order and must not alias the inputs.
 * Same arithmetic contract as the row kernels: child logits, node decisions and hard predictions are bit-equal to theirs
 * on the coerced tensor; P, losses and gradients agree to rounding (the cross-entropy sums run sequentially per pixel
 * here and as a butterfly over lanes there).  nbdt_debug_last_rules_path() reports "pixel".
 * Size limit: R + F <= 640, with R child slots and F the largest fan-out of an inner node -- a pixel's R + F floats of
 * LDS times 64 lanes within 160 KB.  F <= R, so 2R <= 640 always fits; a binary hierarchy fits up to 320 classes
 * (ADE20K: C 150, R 298, F 2).  Every class must lie under at least one child slot.  Beyond it every entry returns NBDT_EINVAL and nbdt_seg_pixel_fits() returns 0: run the
 * row kernels on the coerced tensor (what nbdt.model / nbdt.loss do).  nbdt_set_rules_path does not apply here.
 *
 * nbdt_seg_soft_forward: P [N, C, HW] path probabilities.  One launch.
 * nbdt_seg_soft_backward: gz [N, C, HW] = d<gP, P>/dz, the forward recomputed from z; the path for any criterion that
 *   is not a plain cross entropy.  One launch; gz doubles as the kernel's per-class scratch.
 * nbdt_seg_soft_tree_loss: criterion = nn.CrossEntropyLoss(ignore_index, label_smoothing = smoothing), mean reduction:
 *   loss = w_xent*CE(z, y) + w_tree*CE(P, y), each a mean over the pixels with y != ignore_index (y: [N, HW] int64);
 *   gz = grad_scale * dloss/dz, exactly 0 at ignored pixels.  A label outside [0, C) other than ignore_index gives a NaN
 *   loss; no valid pixel at all gives a NaN loss and a zero gradient, like torch.  THREE launches behind a 4-byte
 *   memset, no host read-back: a count of the valid pixels over y (integer atomics), the main kernel (one row-loss sum
 *   per block of 64 pixels, by a fixed butterfly), and a one-block fold that adds those sums in block order and divides
 *   by the count -- no floating-point atomics, so two calls on the same input give the same bits.
 *   workspace: nbdt_seg_loss_workspace_floats(N, HW) fp32 of scratch; loss: 1 fp32.
 * nbdt_seg_hard_forward: pred [N, HW] int64, optional onehot [N, C, HW] fp32 (NULL: not written).  One launch. */
int nbdt_seg_pixel_fits(const nbdt_tree* t);
int64_t nbdt_seg_loss_workspace_floats(int64_t N, int64_t HW);
int nbdt_seg_soft_forward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                          float* P, void* stream);
int nbdt_seg_soft_backward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                           const float* gP, float* gz, void* stream);
int nbdt_seg_soft_tree_loss(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                            const int64_t* y, int64_t ignore_index, float smoothing, float w_xent, float w_tree,
                            float grad_scale, float* workspace, float* loss, float* gz, void* stream);
int nbdt_seg_hard_forward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                          int64_t* pred, float* onehot, void* stream);

/* Segmentation evaluation in ONE launch (nbdt_version() >= 132; csrc/seg_stats.h): nbdt_tree_stats_accumulate for NCHW
 * logits -- the three predictions of every pixel (backbone argmax, hard walk, argmax of the soft path product) against
 * its label, from one set of child logits in LDS; no [N, C, HW] probability tensor is written.
 *   z, N, HW, zi, zc: as for nbdt_seg_hard_forward.  y: [N, HW] int64 labels (required when a counter is requested).  A
 *   pixel whose label equals ignore_index, or lies outside [0, C), counts NOWHERE.
 *   stats (host pointer, nullable): the struct of nbdt_tree_stats_accumulate with the meanings documented there, per
 *   pixel instead of per sample -- totals[4] (valid pixels, backbone / hard / soft hits), confusion_net / _hard / _soft
 *   [C*C] (entry [label * C + prediction]), node_counts [N_inner * 5], first_error_depth [max_depth + 1].  Every pointer
 *   may be NULL; everything is int64 and ADDED TO.  node_entropy must be NULL (NBDT_EINVAL otherwise): the fixed-point
 *   entropy sums have no per-pixel form.  The first maximum wins in every argmax (class order, slot order).  The soft
 *   prediction is argmax over classes of what nbdt_seg_soft_forward writes, bit for bit; in a multi-parent graph the
 *   product runs over every slot that holds the class, as in nbdt_tree_stats_accumulate.
 *   pred_net / pred_hard / pred_soft (nullable) are WRITTEN as [N, HW] int64: the prediction of every pixel, ignored
 *   ones included, as nbdt_seg_hard_forward does.
 * One launch on a persistent grid, no floating-point atomics, no host read-back; all sums are integer sums, so the
 * counters are bit-identical however the pass is cut into calls.  A block keeps totals, node_counts and
 * first_error_depth in LDS and adds them once; a confusion entry costs one atomic per distinct (label, prediction) pair
 * of a wave's 64 pixels.  nbdt_debug_last_rules_path() reports "pixel".
 * Size limit: the (R + F) * 256 bytes of the pixel form's rows plus 4 * (5 * N_inner + max_depth + 5) bytes of block
 * counters (rounded up to 8) within 160 KB of LDS -- slightly tighter than nbdt_seg_pixel_fits (ADE20K: 75 KB + 3 KB).
 * nbdt_seg_stats_fits() returns 0 beyond it and the entry NBDT_EINVAL: run nbdt_tree_stats_accumulate on the coerced
 * tensor.  Refused with NBDT_EINVAL before any device call: such a hierarchy, y == NULL while a counter is requested,
 * non-NULL node_entropy, nothing requested at all, and tensors past the nbdt_seg_* limits or with N*HW >= 2^31.
 * nbdt_set_seg_stats_max_blocks (process-wide, default 0 = one block per resident wave slot, at most 16 per CU) caps the
 * persistent grid: for tests that want a block to stride over several chunks; negative values are NBDT_EINVAL. */
int nbdt_seg_stats_fits(const nbdt_tree* t);
int nbdt_seg_stats_accumulate(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                              const int64_t* y, int64_t ignore_index, const nbdt_tree_stats* stats, int64_t* pred_net,
                              int64_t* pred_hard, int64_t* pred_soft, void* stream);
int nbdt_set_seg_stats_max_blocks(int blocks);
int nbdt_get_seg_stats_max_blocks(void);

/* ---- cross-entropy on bilinearly upsampled logits (nbdt_version() >= 133; csrc/upsampled_xent.hip, upsample_taps.h):
 *   F.cross_entropy(F.interpolate(x, size=(H, W), mode="bilinear", align_corners), y, weight, ignore_index,
 *                   reduction="mean", label_smoothing = smoothing)
 * and its gradient from the LOW-resolution x and the FULL-resolution labels -- the criterion of backbones whose logits
 * come at 1/4 of the label size.  No tensor of N*C*H*W elements is formed and no floating-point atomic is used: two
 * calls on the same input give the same bits (torch's bilinear backward scatters with atomics).
 *   x: [N, C, h, w] of type xtype (NBDT_F32 / _BF16 / _F16); the h*w elements of a plane are contiguous, image n /
 *   channel c starts at element n*xi + c*xc (so a channel-sliced view works; xc >= h*w, xi >= (C-1)*xc + h*w).
 *   y: [N, H, W] int64.  weight: [C] fp32 class weights or NULL.  gx: [N, C, h, w] dense fp32 = grad_scale * dloss/dx.
 *   workspace: nbdt_upsampled_xent_workspace_floats(N, H, W) fp32 (lse and label per pixel, per-wave partials); loss: 1 fp32.
 * Interpolation contract, per axis with `in` source and `out` destination samples, in fp32, every multiply and add a
 * single rounding (torch's, ATen UpSample.h):
 *   align_corners = 0: scale = (float)in / out,  src = max(scale * (dst + 0.5f) - 0.5f, 0)
 *   align_corners = 1: scale = out > 1 ? (float)(in - 1) / (out - 1) : 0,  src = scale * dst
 *   i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1;  value = ly0*(lx0*a + lx1*b) + ly1*(lx0*c + lx1*d)
 * nbdt_upsample_taps returns exactly what the kernels use for one destination index; nbdt_upsample_footprint the
 * inclusive range of destinations whose taps can touch source index i (out >= in; never short, possibly holding a
 * destination of weight 0).  Neither touches a device.
 * Criterion: without weight, t'_c = (1 - smoothing) * 1[c == y] + smoothing / C, row = lse - sum_c t'_c v_c, mean over
 * the pixels with y != ignore_index; with weight (smoothing must be 0), row = weight[y] * (lse - v_y) and the divisor is
 * the sum of weight[y] over those pixels, in a fixed order.  A label outside [0, C) other than ignore_index gives a NaN
 * loss; no valid pixel gives a NaN loss and a zero gradient.
 * Three launches, no host read-back: forward (one lane per full-resolution pixel), a one-block fold of the per-wave
 * partials in block order, and the gather-form backward (one lane per low-resolution pixel: the ordered sum over the
 * pixels whose taps touch it, v recomputed from its 3 x 3 neighbourhood by the forward's own function).
 * Refused with NBDT_EINVAL before any HIP call: null or aliased buffers, an unknown xtype, empty tensors, H < h or
 * W < w (downsampling), H or W > 2^22, N*H*W >= 2^31, C > 262,140, overlapping planes, smoothing outside [0, 1), weight
 * together with smoothing > 0, a NaN grad_scale. */
int nbdt_upsample_taps(int in, int out, int align_corners, int dst, int* i0, int* i1, float* l0, float* l1);
int nbdt_upsample_footprint(int in, int out, int align_corners, int i, int* lo, int* hi);
int64_t nbdt_upsampled_xent_workspace_floats(int64_t N, int64_t H, int64_t W);
int nbdt_upsampled_xent(const void* x, int xtype, int64_t N, int64_t C, int64_t h, int64_t w, int64_t xi, int64_t xc,
                        const int64_t* y, int64_t H, int64_t W, int align_corners, int64_t ignore_index,
                        const float* weight, float smoothing, float grad_scale, float* workspace, float* loss, float* gx,
                        void* stream);

/* ------------------------------------------------------------------ superclass evaluation (nbdt_version() >= 131)
 * Zero-shot evaluation on superclasses (reference nbdt/analysis.py:430-559, Superclass / SuperclassNBDT) and
 * get_node_logits over an ad-hoc grouping of the classes (nbdt/model.py:84-99 with new_to_old_classes), csrc/superclass.hip.
 *
 * Grouping handle.  G groups over C classes: group g lists the classes group_cls[group_off[g] .. group_off[g+1]), in the
 * order its sums run.  A class may lie in several groups or in none; a group may be empty.  Both arrays are HOST pointers
 * and are copied to `device`, together with the transposed map (class -> the groups holding it, ascending group index)
 * that the backward pass walks.  NBDT_EINVAL with a message: a class twice within one group, a class index outside
 * [0, C), offsets that do not start at 0 or decrease, C <= 0 or G <= 0.
 *
 * Arithmetic contract (that of the rules layer): a group's logit is the sequential fp32 sum of its members in the listed
 * order, starting from 0.0f, followed by one IEEE division by the member count; an empty group gives NaN (0 / 0), as
 * torch's mean of an empty slice does; bf16 / fp16 logits are widened exactly.  A maximum is torch's: NaN is the largest
 * value and the first of equal values wins.  No floating-point atomics: two calls on the same input give the same bits.
 *
 * Size limits: none.  Rows are not staged in LDS whole: the member list is walked in chunks of 2048 entries (8 KB of
 * static LDS), and every row offset (b * ldz, b * G, b * C) is 64-bit.  C = 21,841 runs like C = 10.
 *
 * nbdt_group_logits: out [B, G] fp32, every element written.  z: [B, C] logits of type ztype, row stride ldz >= C.
 * nbdt_group_logits_backward: gz [B, C] fp32 from gs [B, G] fp32: gz[b][c] = the sequential sum, over the groups g
 *   holding c in ascending g and starting from 0.0f, of gs[b][g] / n_g (one division per term, then the add).  A class
 *   in no group gets exactly 0.  gz is WRITTEN, every element, never added to.
 * nbdt_superclass_accumulate: one evaluation batch in ONE launch, no host read-back.
 *   y [B] int64 labels of the TEST label set; map_target int32 [C_test]: test class -> superclass or -1;
 *   map_pred int32 [C]: training class -> superclass or -1 (required by NBDT_SUPER_MASKED, unused otherwise).
 *   mode NBDT_SUPER_MASKED (Superclass.forward): every class with map_pred[c] < 0 takes the value -100.0f (the
 *     reference's constant, not -inf), the first maximum over all C classes wins, and the prediction is
 *     map_pred[argmax]: -1 when every mapped logit lies below -100.
 *   mode NBDT_SUPER_GROUP_MEAN (SuperclassNBDT.forward): the prediction is the first maximum of the G group logits.
 *   Both: t = map_target[y[b]]; a sample with y[b] outside [0, C_test), or with t outside [0, G), counts nowhere;
 *   otherwise totals[0] += 1, totals[1] += (prediction == t), and, when 0 <= prediction < G,
 *   confusion[t * G + prediction] += 1.  pred (nullable) [B] int64 is written for EVERY row, whatever its target.
 *   totals [2] and confusion [G * G] (nullable) are int64 and ADDED TO, never overwritten: the caller zeroes them once
 *   per pass; all sums are integer sums, so any split of the pass into batches gives the same bits. */
#define NBDT_SUPER_MASKED 0
#define NBDT_SUPER_GROUP_MEAN 1
typedef struct nbdt_groups nbdt_groups;
int nbdt_groups_create(int device, int num_classes, int num_groups, const int32_t* group_off, const int32_t* group_cls,
                       nbdt_groups** out);
int nbdt_groups_destroy(nbdt_groups* g);
int nbdt_group_logits(const nbdt_groups* g, const void* z, int ztype, int64_t B, int64_t ldz, float* out, void* stream);
int nbdt_group_logits_backward(const nbdt_groups* g, const float* gs, int64_t B, float* gz, void* stream);
int nbdt_superclass_accumulate(const nbdt_groups* g, const void* z, int ztype, int64_t B, int64_t ldz, const int64_t* y,
                               const int32_t* map_target, int32_t C_test, const int32_t* map_pred, int32_t mode,
                               int64_t* totals, int64_t* confusion, int64_t* pred, void* stream);

/* ------------------------------------------------------------------ backbone: implicit-GEMM conv
 * One launch = one "tap table": out[pix(m)][n] (+)= sum_t sum_c in[pix_in(m) + tap_off[t]][c] *
 * w[n][w_tap[t]][c].  Pixel m of the launch's M-pixel grid decomposes as (b, i, j) over
 * (B, gh, gw); element offsets are affine: b*bs + i*hs + j*ws + base.  This single kernel is
 * Conv2d forward (3x3/1x1, stride 1/2; nbdt/models/resnet.py:47-66), its dgrad (flipped taps,
 * parity classes for stride 2) and the 1x1 shortcut, replacing cuDNN/MIOpen.           */
typedef struct nbdt_conv_desc {
  int32_t B, gh, gw;            /* pixel grid of this launch: M = B*gh*gw */
  int32_t cin, cout;            /* cin % 32 == 0, cout % 32 == 0 */
  int32_t ntaps;                /* <= 9 */
  int32_t tap_off[9];           /* element offset added to the input pixel offset */
  int32_t w_tap[9];             /* tap index into the weight tensor */
  int32_t w_ntaps;              /* taps stored in the weight tensor (row length = w_ntaps*cin) */
  int32_t in_bs, in_hs, in_ws, in_base;      /* element strides of the input pixel map */
  int32_t out_bs, out_hs, out_ws, out_base;  /* element strides of the output pixel map */
  int32_t accumulate;           /* 1: out += result (reads out) */
  int32_t wide_tile;            /* dense 3x3 stride-1 launches with w_tiled: 0 / 1 = pick the tile from the grid size (the
                                   8-wave ping-pong kernel on 512-pixel tiles when they give >= 3/4 of the CUs a block,
                                   on 256-pixel half tiles when those fit the CUs in one round, else 512-pixel tiles);
                                   2 = force 512-pixel tiles (error if the shape does not fit), 3 = force the 4-wave
                                   256-pixel kernel, 4 = force 512-pixel tiles with the padded LDS pitch (images narrower
                                   than 32 pixels: bank-conflict-free halo reads, measured 1-2 % slower, so never picked
                                   automatically), 5 = force half tiles.  2 - 5 exist for tests and A/B measurements. */
  int32_t ksplit;               /* (a reserved, ignored field before nbdt_version() 106: zero-initialise descriptors;
                                   negative values, and n > 1 without wide_tile = 5, are NBDT_EINVAL)
                                   half tiles on at most half the CUs: blocks per output tile, each a range of the 32-channel
                                   input slices (partials through a per-stream fp32 workspace, the last block sums them in
                                   split order and runs the epilogue).  0 = automatic (only with an automatic wide_tile),
                                   1 = never, n = n blocks per tile (tests, A/B; with wide_tile = 5) */
  uint64_t w_tiled;             /* 0, or device pointer to the same weights pre-arranged by nbdt_weight_tile_batched
                                   (only dense 3x3 stride-1 launches with the identity tap map use it) */
} nbdt_conv_desc;
/* Host only, no device work: which kernel form the launches below pick for this descriptor and this process's reserved
 * CUs (nbdt_set_reserved_cus) -- so that the launch rules can be tested and planned with without a GPU.
 * form: 0 = first-generation implicit GEMM (strided / 1x1 / anything that is not a dense 3x3 stride-1 conv over a padded
 * tensor), 1 = 4-wave 256-pixel kernels (no DMA-ordered weights), 2 = ping-pong kernel on 512-pixel tiles, 3 = the same with
 * the padded LDS pitch, 4 = ping-pong kernel on 256-pixel half tiles; ksplit: blocks per half tile the rule asks for
 * (form 4; a launch without its per-stream workspace -- first use inside a hipGraph capture -- runs unsplit). */
int nbdt_conv_plan(const nbdt_conv_desc* d, int32_t* form, int32_t* ksplit);
/* in/out/w bf16; residual (nullable) bf16 addressed like out and added before rounding */
int nbdt_conv_igemm(const nbdt_conv_desc* d, const void* in, const void* w, void* out,
                    const void* residual, void* stream);

/* Up to four nbdt_conv_igemm launches over the SAME operands in one grid (no residual, no statistics; `accumulate`
 * must agree): the output-parity classes of a strided 3x3 data gradient write disjoint pixels, and each alone fills a
 * quarter of the chip at 512 images.  Same arithmetic per descriptor as nbdt_conv_igemm (bit-identical outputs).
 * Replaces the conv-transpose autograd of a strided nn.Conv2d (pytorchcv PreResUnit's first conv of a stage). */
int nbdt_conv_igemm_multi(const nbdt_conv_desc* descs, int32_t n, const void* in, const void* w, void* out,
                          void* stream);

/* ------------------------------------------------------------------ backbone: "slice list" convolutions (round 6)
 * The shape-changing units of a (Wide)ResNet -- a stride-2 3x3 conv, its 1x1 stride-2 shortcut and their data
 * gradients (nbdt/models/resnet.py:56-67; pytorchcv PreResUnit with stride 2 / a channel change behind
 * nbdt/models/wideresnet.py:1-5) -- are not dense 3x3 stride-1 convolutions, but every one of them IS a sum of
 * stride-1 tap-subset convolutions over tensors that share one padded pixel grid:
 *   - the stride-2 forward conv over the space-to-depth copy of its input (nbdt_bn_apply_s2d): phase (p,q) of the
 *     input holds 4 / 2 / 2 / 1 of the nine taps;
 *   - the four output-parity classes of its data gradient over the output gradient (4 / 2 / 2 / 1 taps, strided
 *     stores), the shortcut's data gradient being one more 1-tap term of class (even, even);
 *   - conv2 + shortcut of the same unit: nine taps over conv2's input plus one tap over the unit's (space-to-depth)
 *     input -- the residual add disappears into the K loop.
 * A launch is therefore described as up to four CLASSES (disjoint output pixel maps over the same pixel grid), each an
 * ordered list of 32-channel K SLICES: (input tensor, first channel, tap subset, where its weights are).  One kernel
 * (csrc/conv_seg.hip: 8-wave ping-pong, LDS-resident halo slices, persistent blocks) runs them all.  The plan object
 * owns the device-side step tables (which LDS-DMA piece goes out in which K step); weights are re-tiled into DMA
 * order by nbdt_conv_seg_tile_weights whenever they change. */
typedef struct nbdt_conv_seg_slice {
  int32_t tensor;               /* input tensor index 0..ntensors-1 */
  int32_t ch0;                  /* first of the slice's 32 channels inside a pixel of that tensor (multiple of 8) */
  int32_t ntaps;                /* 1..9 */
  int32_t tap[9];               /* 3*R + S: input pixel (y + R - 1, x + S - 1) of the launch's pixel grid */
  int32_t w_matrix;             /* weight matrix index 0..3 */
  int32_t w_off[9];             /* per tap: element offset, inside a row of that matrix, of the slice's 32 k-values */
} nbdt_conv_seg_slice;
typedef struct nbdt_conv_seg_class {
  int32_t nslices;              /* 1..NBDT_SEG_MAX_SLICES */
  const nbdt_conv_seg_slice* slices;
  int32_t out_bs, out_hs, out_ws, out_base;   /* element strides of the class's output pixel map (like nbdt_conv_desc) */
} nbdt_conv_seg_class;
#define NBDT_SEG_MAX_SLICES 64
typedef struct nbdt_conv_seg_desc {
  int32_t B, gh, gw;            /* pixel grid shared by every input tensor ([B][gh+2][gw+2][pix_stride], zero border)
                                   and by the classes' output maps */
  int32_t cout;                 /* multiple of 32; rows of every weight matrix */
  int32_t ntensors;             /* 1..2: the kernel reads two input tensors; nbdt_conv_seg_create refuses more */
  int32_t pix_stride[4];        /* elements per pixel of each input tensor (entries past ntensors unused) */
  int32_t nmatrices;            /* 1..4 */
  int32_t w_row_stride[4];      /* elements per row of each weight matrix ([cout][row_stride] bf16) */
  int32_t nclasses;             /* 1..4 */
  nbdt_conv_seg_class cls[4];
  int32_t tile;                 /* 0 = pick (512-pixel tiles when they give >= 3/4 of the CUs a block, else 256), 512, 256 */
  int32_t nbuf;                 /* 0 = pick (2 halo buffers when every slice but a class's last has >= 2 taps, else 3), 2, 3 */
} nbdt_conv_seg_desc;
/* Host side only (no GPU needed until the first launch allocates the device tables): validates the description, picks
 * tile / buffers, schedules the LDS-DMA pieces of every slice over the K steps before it; NBDT_EINVAL when the shape
 * does not fit (tiles must be whole image rows / whole images, the halo buffers + weight ring must fit in 160 KB). */
int nbdt_conv_seg_create(const nbdt_conv_seg_desc* d, void** plan);
int nbdt_conv_seg_destroy(void* plan);
/* what the plan chose: tile pixels, halo buffers, K steps per class (steps[4]), max LDS-DMA rounds in one step, bf16
 * elements of the DMA-ordered weight buffer */
int nbdt_conv_seg_info(void* plan, int32_t* tile, int32_t* nbuf, int32_t* steps, int32_t* max_rounds,
                       int64_t* w_tile_elems);
/* w[nmatrices] bf16 device pointers -> w_tiles (w_tile_elems bf16): per class, per cout tile, per K step one
 * (32*NT rows) x 32 k tile stored as the swizzled LDS image it will be copied to */
int nbdt_conv_seg_tile_weights(void* plan, const void* const* w, void* w_tiles, void* stream);
/* in[ntensors] bf16 device pointers; residual (nullable) is addressed like class 0's output; bn_partials (nullable,
 * single-class launches only) as in nbdt_conv_igemm_stats */
int nbdt_conv_seg(void* plan, const void* const* in, const void* w_tiles, void* out, const void* residual,
                  float* bn_partials, void* stream);
/* host copy of one class's K-step records (8 int32 each: tap offset in halo pixels, halo buffer byte offset, LDS-DMA
 * rounds issued in the step, their LDS destination, first halo pixel, channel, tensor, strict flag) and the number of
 * slices its tiles load in their prologue -- so that the DMA schedule can be checked without a GPU.  Returns the
 * number of steps (>= 0) or an error (< 0). */
int nbdt_conv_seg_steps(void* plan, int32_t cls, int32_t* out8, int32_t max_steps, int32_t* npro);

/* same launch, and the epilogue also writes the per-channel sum / sum of squares of the (bf16) output
 * of every 256-pixel tile to bn_partials[ceil(M/256)][2][cout] (plain stores, fully overwritten) -- the
 * statistics the following BatchNorm needs, so nbdt_bn_finalize can replace nbdt_bn_stats (no second
 * pass over the tensor). */
int nbdt_conv_igemm_stats(const nbdt_conv_desc* d, const void* in, const void* w, void* out,
                          const void* residual, float* bn_partials, void* stream);

/* data-gradient launch whose output is dL/d(relu(bn(x))): the epilogue also reads x (the BatchNorm's
 * forward input, same geometry as `out`) and writes per-tile partial sums of g' and g'*xhat, g' = out *
 * [bn(x) > 0] -- the reductions of the BatchNorm backward (nbdt_bn_bwd_fold folds them; replaces
 * nbdt_bn_bwd_reduce and one full re-read of the gradient tensor). */
int nbdt_conv_igemm_bnbwd(const nbdt_conv_desc* d, const void* in, const void* w, void* out,
                          const void* bn_x, const float* save_mean, const float* save_rstd,
                          const float* gamma, const float* beta, float* bn_partials, void* stream);
/* inference: eval-mode BatchNorm folded into per-channel scale/shift (scale = gamma/sqrt(running_var+eps),
 * shift = beta - running_mean*scale) and the activation applied in the conv epilogue:
 *   out = act(conv(in) * scale[c] + shift[c] [+ residual]),  act: NBDT_ACT_NONE | RELU | SWISH.
 * Replaces Conv2d -> BatchNorm2d(eval) -> ReLU [-> += shortcut] of nbdt/models/resnet.py:69-74 in ONE launch. */
int nbdt_conv_igemm_affine(const nbdt_conv_desc* d, const void* in, const void* w, void* out,
                           const void* residual, const float* scale, const float* shift, int32_t act,
                           void* stream);

/* stride-1 1x1 convolution as a GEMM (nbdt_version() >= 113): out[pix(m)][n] (+)= sum_c in[pix(m)][c] * w[n][c] over the
 * B*gh*gw interior pixels of padded NHWC tensors -- conv1 / conv3 of the reference's Bottleneck block, forward (w =
 * [cout][1][cin]) and data gradient (w = the transposed copy [cin][1][cout] nbdt_weight_prep builds).  Replaces
 * nn.Conv2d(kernel_size=1) of nbdt/models/resnet.py:82, 88-90 and its autograd.  Takes the descriptors of a stride-1
 * 1x1 launch of nbdt_conv_igemm and requires ntaps == w_ntaps == 1, in_ws == cin, out_ws == cout, cin % 32 == 0,
 * cout % 32 == 0 and 16-byte aligned pixel offsets; anything else (a strided 1x1, a 3x3, a null pointer) is NBDT_EINVAL,
 * decided before the first launch.  bf16 operands, fp32 accumulation over all of cin in ascending order, one rounding
 * at the store; accumulate = 1 reads out, adds in fp32 and rounds once.  Only interior pixels are written (the halo
 * ring of out keeps its bytes) and the halo of in is never read.  bn_partials (nullable; NBDT_EINVAL together with
 * accumulate): per-channel sum and sum of squares of the bf16 outputs of every 256-pixel tile, to
 * bn_partials[ceil(M/256)][2][cout] exactly as nbdt_conv_igemm_stats writes them (plain stores, every row fully
 * overwritten, run-to-run identical bits; nbdt_bn_finalize folds them).  wide_tile, ksplit and w_tiled are ignored.
 * No residual operand, no eval-affine and no BatchNorm-backward epilogue: those stay with nbdt_conv_igemm_*. */
int nbdt_conv_pw(const nbdt_conv_desc* d, const void* in, const void* w, void* out,
                 float* bn_partials /* nullable */, void* stream);

/* ------------------------------------------------------------------ grouped 3x3 convolution (nbdt_version() >= 125)
 * conv2 of torchvision's ResNeXt Bottleneck (nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)) and its
 * autograd: cin == cout == width, width % 32 == 0, cg = width / groups channels per group with cg in {4, 8, 16, 32}.
 * cg divides 32, so the conv is width / 32 independent dense 32 -> 32 convolutions with block-diagonal weights
 * (csrc/conv_group.hip).  Every tensor is padded NHWC [B][H+2][W+2][width] with a zero ring, B, H, W the conv's INPUT
 * batch and sides (the output is [B][H/stride+2][W/stride+2][width]); stride 1 or 2 with pad 1, even sides at stride 2.
 * Only interior pixels are written: the ring of every output keeps its bytes.  Every argument is checked before the
 * first HIP call (NBDT_EINVAL and a message): null pointers, width % 32 != 0, any other cg (cg = 64 -- layer4 of
 * resnext101_32x8d -- included), any other stride, an odd side at stride 2, an empty batch.
 *
 * nbdt_conv_group_weight_prep: fp32 master w[width][9][cg] ([cout][taps][cin in group]) -> bf16 blocks
 *   wf[width/32][32 co][9][32 ci], explicit zeros off the group diagonal (nullable), and the data-gradient blocks
 *   wd[width/32][32 ci][9][32 co] with the tap order reversed, wd[n][ci][t][co] = wf[n][co][8 - t][ci] (nullable).
 * nbdt_conv_group_weight_prep_batched: the same for n_layers convs in one launch; table (device, int64 [n_layers][5])
 *   rows are {master offset in flat, offset of the layer's blocks in wf_flat / wd_flat, width, cg, index of the
 *   layer's first block}, first blocks ascending from 0, total_blocks = sum of width / 32 (rows are not validated). */
int nbdt_conv_group_weight_prep(const float* w, int32_t width, int32_t cg, void* wf_bf16, void* wd_bf16, void* stream);
int nbdt_conv_group_weight_prep_batched(const float* flat, const int64_t* table, int32_t n_layers, int64_t total_blocks,
                                        void* wf_flat, void* wd_flat, void* stream);
/* out = conv3x3(in), bf16 operands, fp32 accumulation in tap order, one round-to-nearest-even at the store.  scale and
 * shift (both or neither; fp32 [width]): out = act(acc * scale[c] + shift[c]) with the meaning of
 * nbdt_conv_igemm_affine (act: NBDT_ACT_NONE | RELU | SWISH; without scale / shift only NBDT_ACT_NONE).  No residual
 * operand and no statistics epilogue. */
int nbdt_conv_group_fwd(const void* in, const void* wf, void* out, int32_t B, int32_t H, int32_t W, int32_t width,
                        int32_t cg, int32_t stride, const float* scale, const float* shift, int32_t act, void* stream);
/* gin[B][H+2][W+2] = data gradient of the above from gout[B][H/stride+2][W/stride+2], gather form over wd: at stride 2
 * an input pixel sums only the taps its parity allows (4 / 2 / 2 / 1).  accumulate must be 0: there is no
 * accumulating form (NBDT_EINVAL). */
int nbdt_conv_group_dgrad(const void* gout, const void* wd, void* gin, int32_t B, int32_t H, int32_t W, int32_t width,
                          int32_t cg, int32_t stride, int32_t accumulate, void* stream);
/* dw[width][9][cg] fp32 += sum over pixels of gout[p][co] * x[stride p + tap][ci], ci in co's group.  No fp32 atomics:
 * per-pixel-split sums in plain stores to a per-(device, stream) workspace (NBDT_ENOMEM if it cannot be had), then one
 * fold that adds them in split order ONTO what dw holds.  Two runs leave identical bits. */
int nbdt_conv_group_wgrad(const void* x, const void* gout, float* dw, int32_t B, int32_t H, int32_t W, int32_t width,
                          int32_t cg, int32_t stride, void* stream);
/* verification-only fp32-storage twins of the three (see nbdt_ref_conv below): fp32 tensors, w = the fp32 MASTER
 * [width][9][cg] itself (no expansion), one thread per output, direct loops */
int nbdt_ref_conv_group_fwd(const float* in, const float* w, float* out, int32_t B, int32_t H, int32_t W, int32_t width,
                            int32_t cg, int32_t stride, void* stream);
int nbdt_ref_conv_group_dgrad(const float* gout, const float* w, float* gin, int32_t B, int32_t H, int32_t W,
                              int32_t width, int32_t cg, int32_t stride, int32_t accumulate, void* stream);
int nbdt_ref_conv_group_wgrad(const float* x, const float* gout, float* dw, int32_t B, int32_t H, int32_t W,
                              int32_t width, int32_t cg, int32_t stride, void* stream);

/* weight gradient (replaces cuDNN wgrad): dw[cout][w_ntaps][cin] fp32 += sum over the pixel grid
 * of gy[pix_g(m)][co] * x[pix_x(m) + tap_off[t]][ci]; split over pixels with fp32 atomics, so dw
 * must be zeroed (or hold the running .grad) before the call. */
typedef struct nbdt_wgrad_desc {
  int32_t B, gh, gw;
  int32_t cin, cout;
  int32_t ntaps;
  int32_t tap_off[9];
  int32_t w_tap[9];
  int32_t w_ntaps;
  int32_t x_bs, x_hs, x_ws, x_base;
  int32_t g_bs, g_hs, g_ws, g_base;
  int32_t variant;              /* dense 3x3 stride-1 launches: 0 = pick from the problem size (the K-split 8-wave kernel
                                   from 64 pixel stages on, else the 4-wave one); 2 = force the tap-split 8-wave kernel
                                   (two wave groups, taps divided between them), 3 = force the 4-wave one, 4 = force the
                                   12-wave kernel (three wave groups, one kernel row each), 5 = force the K-split 8-wave
                                   kernel (every wave all nine taps, the groups halve the pixels) -- tests, A/B */
  int32_t cu_budget;            /* dense 3x3 stride-1 launches: 0 = size the pixel split for all 256 CUs; n = for n of
                                   them (32..256), so that an HBM-bound pass launched on another stream keeps the
                                   rest: a weight-gradient block takes a CU's whole register file, the two kernels
                                   never share one (probes/cu_share_probe.hip) */
} nbdt_wgrad_desc;
int nbdt_conv_wgrad(const nbdt_wgrad_desc* d, const void* x, const void* gy, float* dw,
                    void* stream);
/* thread blocks the launch above will use for this descriptor (its cu_budget included) when it takes the 8-wave dense
 * 3x3 kernel -- one block per CU, so 256 minus this is what a concurrent HBM-bound pass may take
 * (nbdt_bn_bwd_apply_cus); 0 for every other kernel.  No device work. */
int nbdt_conv_wgrad_blocks(const nbdt_wgrad_desc* d);

/* fp32 master [cout][taps][cin] -> bf16 copy in the same order, and (optional) the dgrad copy
 * wd[cin][taps][cout] with the tap order reversed (wd[ci][t][co] = w[co][taps-1-t][ci]) */
int nbdt_weight_prep(const float* w, int32_t cout, int32_t taps, int32_t cin, void* w_bf16,
                     void* wd_bf16, void* stream);

/* the dgrad copies of EVERY conv layer in one launch: table (device, int64 [n_layers][6]) rows are
 * {src offset in flat, dst offset in wd_flat, cout, taps, cin, first tile index}; cout, cin % 32 == 0; a tile
 * is 64 couts x 32 cins of one tap: total_tiles = sum over layers of taps * ceil(cout/64) * cin/32 */
int nbdt_weight_prep_batched(const float* flat, const int64_t* table, int32_t n_layers, int64_t total_tiles,
                             void* wd_flat, void* stream);

/* ------------------------------------------------------------------ backbone: batch-norm / elementwise
 * Replaces nn.BatchNorm2d (train mode, eps 1e-5, momentum 0.1) + F.relu + residual adds
 * (nbdt/models/resnet.py:69-74; pytorchcv PreResUnit) and their autograd.  Tensors are padded
 * NHWC bf16 [B][H+2][W+2][C], C % 8 == 0; only interiors are read/written.  `scratch` is
 * NBDT_BN_SLOTS*2*C fp32 of caller-owned workspace that must be ZERO on entry; every call leaves it
 * zero again (the fold kernel clears what it read), so one zero-initialised buffer serves all layers. */
#define NBDT_BN_SLOTS 32
/* batch statistics: save_mean/save_rstd [C]; updates running_mean/var (unbiased var) if non-NULL.
 * x == NULL: only fold sums a producer already left in `scratch` (nbdt_dwconv_fwd with bn_scratch). */
int nbdt_bn_stats(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, float eps,
                  float momentum, float* running_mean, float* running_var, float* scratch,
                  float* save_mean, float* save_rstd, void* stream);
/* fold the partial sums nbdt_conv_igemm_stats wrote for a [B,H,W,C] output (ceil(B*H*W/256) rows) into
 * save_mean/save_rstd + running statistics */
int nbdt_bn_finalize(int32_t B, int32_t H, int32_t W, int32_t C, float eps, float momentum,
                     float* running_mean, float* running_var, const float* bn_partials, float* save_mean,
                     float* save_rstd, void* stream);
/* y = relu?( (x-mean)*rstd*gamma + beta [+ residual] ) */
int nbdt_bn_apply(const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                  const float* beta, const void* residual, int32_t relu, int32_t B, int32_t H,
                  int32_t W, int32_t C, void* y, void* stream);
/* the same pass writing the SPACE-TO-DEPTH copy of its output: y is [B][H/2+2][W/2+2][4C] bf16 (zero border), input
 * pixel (h, w) at pixel (h/2, w/2), channels [((h&1)*2 + (w&1))*C, +C).  What the stride-2 conv1 and the 1x1 stride-2
 * shortcut of a shape-changing unit (and their weight gradients) read instead of the plain activated tensor:
 * pytorchcv PreResUnit's shared pre-activation (nbdt/models/wideresnet.py:1-5), nbdt/models/resnet.py:56-67. */
int nbdt_bn_apply_s2d(const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                      const float* beta, int32_t relu, int32_t B, int32_t H, int32_t W, int32_t C, void* y,
                      void* stream);
/* backward, pass 1: with gy' = gy * mask when relu, writes dsum[0][c] = sum gy',
 * dsum[1][c] = sum gy' * xhat and accumulates dbeta += dsum[0], dgamma += dsum[1] (either may be
 * NULL).  mask = (y > 0) from the stored forward output y; with y == NULL (no residual in the
 * forward) it is recomputed from x, gamma, beta with bn_apply's own expression -- one tensor read less. */
int nbdt_bn_bwd_reduce(const void* gy, const void* y, const void* x, const float* save_mean,
                       const float* save_rstd, const float* gamma, const float* beta, int32_t relu,
                       int32_t B, int32_t H, int32_t W, int32_t C, float* scratch, float* dsum,
                       float* dgamma, float* dbeta, void* stream);
/* fold the partials of nbdt_conv_igemm_bnbwd into dsum[2][C]; dbeta += dsum[0], dgamma += dsum[1] */
int nbdt_bn_bwd_fold(int32_t B, int32_t H, int32_t W, int32_t C, const float* bn_partials, float* dsum,
                     float* dgamma, float* dbeta, void* stream);
/* backward, pass 2: gx = gamma*rstd*(gy' - (dsum0 + xhat*dsum1)/N) [+ gx_add];
 * g_resid (nullable) receives gy' (the gradient of the residual input). */
int nbdt_bn_bwd_apply(const void* gy, const void* y, const void* x, const float* save_mean,
                      const float* save_rstd, const float* gamma, const float* beta, const float* dsum,
                      const void* gx_add, int32_t relu, int32_t B, int32_t H, int32_t W, int32_t C,
                      void* gx, void* g_resid, void* stream);
/* nbdt_bn_bwd_apply with relu = 1, y = NULL, g_resid = NULL on `cus` CUs only (one persistent block each): the pass is
 * HBM-bound and needs few of them (64 CUs stream 3.0 TB/s, 96 4.1 TB/s, all 256 5.6 TB/s), so an MFMA-bound launch on
 * another stream -- nbdt_conv_wgrad with nbdt_wgrad_desc.cu_budget = 256 - cus -- runs on the rest at the same
 * time.  (Blocks of the ordinary launch land on every CU and keep a weight-gradient block, which takes a CU's whole
 * register file, from starting.)  Same arithmetic, same results as nbdt_bn_bwd_apply. */
int nbdt_bn_bwd_apply_cus(const void* gy, const void* x, const float* save_mean, const float* save_rstd,
                          const float* gamma, const float* beta, const float* dsum, const void* gx_add,
                          int32_t B, int32_t H, int32_t W, int32_t C, void* gx, int32_t cus, void* stream);
/* nbdt_bn_bwd_reduce with relu = 1, y = NULL on `cus` CUs only (see nbdt_bn_bwd_apply_cus): with it the sums need not
 * come out of the data gradient's epilogue (nbdt_conv_igemm_bnbwd), and the whole BatchNorm backward -- reduce, fold,
 * apply -- is HBM-bound work that runs beside the weight gradient.  scratch: the zeroed 32-slot buffer of
 * nbdt_bn_bwd_reduce (left zeroed). */
int nbdt_bn_bwd_reduce_cus(const void* gy, const void* x, const float* save_mean, const float* save_rstd,
                           const float* gamma, const float* beta, int32_t B, int32_t H, int32_t W, int32_t C,
                           float* scratch, float* dsum, float* dgamma, float* dbeta, int32_t cus, void* stream);
/* nbdt_bn_bwd_reduce_cus + nbdt_bn_bwd_apply_cus as TWO launches instead of three: the fold of the 32 slots
 * (bn_bwd_finalize, 7 us on the backward critical path of every conv) happens in the prologue of the elementwise pass --
 * every block folds the slots for itself, block 0 writes dsum / accumulates dgamma, dbeta.  The slots being read cannot
 * be re-zeroed inside that launch, so the caller passes a PAIR of 32-slot buffers and alternates them from call to
 * call: `slots` (zero on entry, dirty on return) receives this call's sums, `slots_other` (not touched by anyone
 * while this call runs) is left zeroed for the next call.  Same arithmetic and summation order as the three-launch
 * form: bit-identical gx / dsum in deterministic mode.  Replaces the autograd of F.relu(bn(x)) (pytorchcv
 * PreResActivation behind nbdt/models/wideresnet.py:1-5). */
int nbdt_bn_bwd_cus(const void* gy, const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                    const float* beta, const void* gx_add, int32_t B, int32_t H, int32_t W, int32_t C, float* slots,
                    float* slots_other, float* dsum, float* dgamma, float* dbeta, void* gx, int32_t cus,
                    void* stream);
/* head: pooled[b][c] = mean over (h,w) of relu(bn(x))  (post_activ + final_pool / avg_pool2d,
 * nbdt/models/resnet.py:142) and its backward given gpooled[B][C] (same two passes) */
int nbdt_bn_relu_pool(const void* x, const float* save_mean, const float* save_rstd,
                      const float* gamma, const float* beta, int32_t B, int32_t H, int32_t W,
                      int32_t C, float* pooled, void* stream);
int nbdt_pool_bn_bwd_reduce(const float* gpooled, const void* x, const float* save_mean,
                            const float* save_rstd, const float* gamma, const float* beta,
                            int32_t B, int32_t H, int32_t W, int32_t C, float* scratch, float* dsum,
                            float* dgamma, float* dbeta, void* stream);
int nbdt_pool_bn_bwd_apply(const float* gpooled, const void* x, const float* save_mean,
                           const float* save_rstd, const float* gamma, const float* beta,
                           const float* dsum, int32_t B, int32_t H, int32_t W, int32_t C, void* gx,
                           void* stream);

/* ------------------------------------------------------------------ backbone: MBConv pieces (EfficientNet-B0)
 * Replaces pytorchcv `efficientnet_b0` building blocks behind nbdt/models/__init__.py:3:
 * dwconv{3x3,5x5}_block, BatchNorm2d + Swish, SEBlock, Dropout -- and their autograd.  Same padded NHWC
 * bf16 tensors as above.  The activated tensor a = act(bn(x)) is never stored for the SE branch: every
 * pass recomputes it from the raw conv output x and the saved batch statistics. */
#define NBDT_ACT_NONE 0
#define NBDT_ACT_RELU 1
#define NBDT_ACT_SWISH 2
/* y = act(bn(x)) [* gate[b][c]] [+ residual]        gate: fp32 [B][C] or NULL */
int nbdt_bn_act_apply(const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                      const float* beta, int32_t act, const float* gate, const void* residual, int32_t B,
                      int32_t H, int32_t W, int32_t C, void* y, void* stream);
/* out[b][c] = scale * sum_hw act(bn(x)) [* mul]      (SE squeeze / head average pool with scale = 1/HW;
 * with mul = upstream gradient and scale = 1: dL/dgate of the SE scaling).  out: fp32 [B][C], overwritten */
int nbdt_bn_act_pool(const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                     const float* beta, int32_t act, const void* mul, float scale, int32_t B, int32_t H,
                     int32_t W, int32_t C, float* out, void* stream);
/* backward of u = act(bn(x)) * gate (+ the pooled branch) w.r.t. x, gamma, beta in two passes:
 *   gradient entering the activation g_a = gu                               (gate == NULL, gu != NULL)
 *                                        = gu*gate[b][c] + gpool[b][c]/HW   (SE form)
 *                                        = gpool[b][c]/HW                    (gu == NULL: average-pool head)
 * dgamma/dbeta are accumulated (+=); gx [+= gx_add]; scratch/dsum as in nbdt_bn_bwd_reduce. */
int nbdt_bn_act_bwd(const void* gu, const float* gate, const float* gpool, const void* x,
                    const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                    int32_t act, const void* gx_add, int32_t B, int32_t H, int32_t W, int32_t C,
                    float* scratch, float* dsum, float* dgamma, float* dbeta, void* gx, void* stream);
/* depthwise Conv2d(C, C, k in {3,5}, stride in {1,2}, padding k/2, groups=C): x [B][H+2][W+2][C] ->
 * y [B][H/stride+2][W/stride+2][C]; w fp32 [k*k][C] (tap-major); dw accumulated (+=). */
int nbdt_dwconv_fwd(const void* x, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                    int32_t stride, void* y, float* bn_scratch /* nullable: also accumulate sum(y), sum(y^2)
                    into the NBDT_BN_SLOTS scratch for nbdt_bn_stats(x = NULL, ...) */, void* stream);
int nbdt_dwconv_bwd_data(const void* gy, const float* w, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t k, int32_t stride, void* gx, void* stream);
/* Stride-1 depthwise data gradient whose epilogue also produces the backward sums of the BatchNorm + swish that fed the
 * depthwise conv (MBConv: dwconv(swish(bn1(e))) -- pytorchcv dwconv block after the expand conv): gx = dL/d(swish(bn(bn_x))),
 * and sum(g'), sum(g' * xhat) with g' = gx * swish'(bn(bn_x)) go to the 32-slot `scratch` -- follow with
 * nbdt_bn_act_bwd_apply (fold + elementwise pass), which replaces nbdt_bn_act_bwd's reduction pass over gx and bn_x. */
int nbdt_dwconv_bwd_data_bn(const void* gy, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                            void* gx, const void* bn_x, const float* save_mean, const float* save_rstd,
                            const float* gamma, const float* beta, float* scratch, void* stream);
/* nbdt_bn_act_bwd without its reduction pass: the sums are already in `scratch` (plain form only: no gate, no pool). */
int nbdt_bn_act_bwd_apply(const void* gu, const void* x, const float* save_mean, const float* save_rstd,
                          const float* gamma, const float* beta, int32_t act, const void* gx_add, int32_t B, int32_t H,
                          int32_t W, int32_t C, float* scratch, float* dsum, float* dgamma, float* dbeta, void* gx,
                          void* stream);
/* Squeeze-and-excitation backward with ONE reduction pass over (gu, x) instead of two (nbdt_bn_act_pool(mul = gu) for
 * dL/dgate, then nbdt_bn_act_bwd's sums).  The gradient entering the activation, g_a = gu*gate[b][c] + gpool[b][c]/HW, is
 * linear in (gate, gpool) per image and channel, so the BatchNorm-backward sums follow from five per-(image, channel) sums
 * that do not need gpool: sums[5][B][C] fp32 += { sum gu*act(y), sum gu*act'(y), sum gu*act'(y)*xhat, sum act'(y),
 * sum act'(y)*xhat } over the image's pixels, y = bn(x).  `sums` must be ZERO on entry (allocate it zeroed once); sums[0]
 * is dL/dgate: feed it to nbdt_se_gate_bwd, then nbdt_bn_act_se_bwd_apply folds sums[1..4] with gate / gpool into dsum
 * (dgamma, dbeta accumulate), ZEROES `sums` again for the next use (no memset launch per call) and runs
 * nbdt_bn_act_bwd's elementwise pass.  Replaces the autograd of pytorchcv's SEBlock scaling + BatchNorm + swish
 * (reference: nbdt/models/__init__.py:3).  Not available in deterministic mode (atomics across pixel slices). */
int nbdt_bn_act_se_sums(const void* gu, const void* x, const float* save_mean, const float* save_rstd,
                        const float* gamma, const float* beta, int32_t act, int32_t B, int32_t H, int32_t W, int32_t C,
                        float* sums, void* stream);
int nbdt_bn_act_se_bwd_apply(const void* gu, const float* gate, const float* gpool, float* sums, const void* x,
                             const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                             int32_t act, int32_t B, int32_t H, int32_t W, int32_t C, float* dsum, float* dgamma,
                             float* dbeta, void* gx, void* stream);
int nbdt_dwconv_bwd_weight(const void* x, const void* gy, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t k, int32_t stride, float* dw, void* stream);
/* SEBlock gate: gate[b][c] = sigmoid(W2 swish(W1 pooled[b] + b1) + b2) for c < C_real, 0 above.
 * pooled/gate rows have stride C; W1 [S][C_real], W2 [C_real][S]; pre1 [B][S] saved for backward. */
int nbdt_se_gate_fwd(const float* pooled, const float* w1, const float* b1, const float* w2,
                     const float* b2, int32_t B, int32_t C, int32_t C_real, int32_t S, float* pre1,
                     float* gate, void* stream);
/* dgate [B][C] -> gpool [B][C] (gradient of the pooled mean) and += dW1, db1, dW2, db2;
 * dpre2 [B][C_real], dpre1 [B][S]: workspaces.  dw1 = db1 = dw2 = db2 = NULL: the data part only -- the parameter
 * gradients (which feed nothing but the optimizer) are then the caller's to launch, e.g. on a second stream, with
 * nbdt_se_param_grad on the dpre2 / dpre1 this call left (nbdt_version() >= 108). */
int nbdt_se_gate_bwd(const float* dgate, const float* gate, const float* pre1, const float* pooled,
                     const float* w1, const float* w2, int32_t B, int32_t C, int32_t C_real, int32_t S,
                     float* dpre2, float* dpre1, float* gpool, float* dw1, float* db1, float* dw2,
                     float* db2, void* stream);
int nbdt_se_param_grad(const float* dpre2, const float* dpre1, const float* pre1, const float* pooled,
                       int32_t B, int32_t C, int32_t C_real, int32_t S, float* dw1, float* db1, float* dw2,
                       float* db2, void* stream);
/* nn.Dropout(p) on n fp32 values: mask[i] in {0,1} from a counter hash of (seed, i); y = x*mask/(1-p).
 * n <= 256 * (2^31 - 1): one block per 256 elements (NBDT_EINVAL beyond). */
int nbdt_dropout_fwd(const float* x, int64_t n, float p, uint32_t seed, uint8_t* mask, float* y,
                     void* stream);
int nbdt_dropout_bwd(const float* gy, int64_t n, float p, const uint8_t* mask, float* gx, void* stream);

/* ---- stochastic depth (nbdt_version() >= 122): torchvision's StochasticDepth(p, mode="row") on the branch of an MBConv
 * residual add, inside the passes that exist already.  Replaces `stochastic_depth(...)` behind torchvision's
 * efficientnet_b0 MBConv.forward; the reference's pytorchcv model has none.
 *
 * nbdt_bn_act_apply_rows: y = residual + row_scale[b] * act(bn(x)), row_scale fp32 [B] (device).  The statistics are the
 * whole batch's: the scale comes after the BatchNorm.  A factor of exactly 0 copies the residual's bits; a factor of 1
 * gives the bits of nbdt_bn_act_apply.  row_scale needs a residual and takes no gate: anything else is NBDT_EINVAL before
 * any launch (gate is in the signature only to be refused).
 *
 * nbdt_bn_act_bwd_rows: nbdt_bn_act_bwd's plain form with g_a = gu * row_scale[b]: a dropped image adds exact zeros to
 * the sums and still receives gx = gamma*rstd * (-mean(g_y) - xhat * mean(g_y*xhat)) [+ gx_add] through the batch
 * statistics.  The skip gradient is the caller's (gu itself, unscaled).  gu == NULL, a gate or a gpool is NBDT_EINVAL
 * before any launch.  scratch is left zero and deterministic mode holds as for nbdt_bn_act_bwd. */
int nbdt_bn_act_apply_rows(const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                           const float* beta, int32_t act, const float* gate, const void* residual,
                           const float* row_scale, int32_t B, int32_t H, int32_t W, int32_t C, void* y, void* stream);
int nbdt_bn_act_bwd_rows(const void* gu, const float* row_scale, const float* gate, const float* gpool, const void* x,
                         const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                         int32_t act, const void* gx_add, int32_t B, int32_t H, int32_t W, int32_t C, float* scratch,
                         float* dsum, float* dgamma, float* dbeta, void* gx, void* stream);
/* The factors of one training forward in ONE launch: table[U][B] fp32 (device) = u < prob[unit] ? 0 : scale[unit].
 * prob / scale: HOST fp32 [U], U <= NBDT_SD_MAX_UNITS, 0 <= prob < 1, scale finite and > 0 (the caller rounds
 * 1 / (1 - prob) to fp32 once, so no bit depends on the device's division); they travel as kernel arguments.  A unit
 * without a skip has prob 0 and scale 1: its row is all ones.  The draw is a pure function of
 * (seed, stream_id, counter, unit, image) -- not of B.  With mix64 (splitmix64's finaliser) as for nbdt_augment_batch,
 * G = 0x9E3779B97F4A7C15 and K = 0xD1342543DE82EF95, all arithmetic mod 2^64:
 *   key = mix64(mix64(seed * G + counter) ^ (stream_id * K))
 *   r   = mix64(key ^ ((unit << 32 | image) * K)),   u = (float)(r >> 40) * 2^-24   (exact, in [0, 1))
 * nbdt/ops.py draw_stochastic_depth restates it with numpy, bit for bit. */
#define NBDT_SD_MAX_UNITS 64
int nbdt_stochastic_depth_draw(uint64_t seed, uint64_t stream_id, uint64_t counter, const float* prob,
                               const float* scale, int32_t U, int32_t B, float* table, void* stream);

/* ------------------------------------------------------------------ verification-only fp32-storage kernels
 * NOT the product path (csrc/ref_fp32.hip): the same operators as above on fp32 padded NHWC tensors, written to be
 * obviously right (one thread per output, plain loops, double accumulators), taking the SAME descriptors.  The engines'
 * fp32 reference mode (engine.set_reference_fp32) routes every launch here while keeping its launch order, streams,
 * events and buffer rotation, so that ONE test can show the whole training step -- in the shipped schedule -- agreeing
 * with the fp32 oracle to 1e-5 instead of the cosine ~0.9 that bf16 storage allows (tests/test_reference_fp32_gpu.py).
 * They replace, for verification, the same reference lines as their product twins (nbdt/models/resnet.py:47-74,
 * 115-149; pytorchcv PreResUnit). */
int nbdt_ref_conv(const nbdt_conv_desc* d, const float* in, const float* w, float* out, const float* residual,
                  void* stream);
int nbdt_ref_wgrad(const nbdt_wgrad_desc* d, const float* x, const float* gy, float* dw, void* stream);
/* twin of nbdt_conv_seg: fp32 tensors, fp32 weight matrices in their plain [cout][row_stride] layout (no tiling) */
int nbdt_ref_conv_seg(void* plan, const float* const* in, const float* const* w, float* out, const float* residual,
                      void* stream);
/* partials == NULL: nbdt_bn_stats.  partials != NULL: the conv-epilogue form -- row 0 of bn_partials[rows][2][C]
 * receives sum / sum of squares, the other rows zero (nbdt_bn_finalize folds them as usual). */
int nbdt_ref_bn_stats(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, float eps, float momentum,
                      float* running_mean, float* running_var, float* save_mean, float* save_rstd, float* partials,
                      void* stream);
int nbdt_ref_bn_apply(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                      const float* beta, const float* residual, int32_t relu, int32_t B, int32_t H, int32_t W,
                      int32_t C, float* y, void* stream);
int nbdt_ref_bn_apply_s2d(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                          const float* beta, int32_t relu, int32_t B, int32_t H, int32_t W, int32_t C, float* y,
                          void* stream);
/* nbdt_bn_bwd_reduce + nbdt_bn_bwd_apply (gy given) or nbdt_pool_bn_bwd_reduce + _apply (gy NULL, gpooled given);
 * reduce == 0: the elementwise pass only, with the caller's dsum */
int nbdt_ref_bn_bwd(const float* gy, const float* gpooled, const float* y, const float* x, const float* save_mean,
                    const float* save_rstd, const float* gamma, const float* beta, int32_t relu, const float* gx_add,
                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t reduce, float* dsum, float* dgamma,
                    float* dbeta, float* gx, float* g_resid, void* stream);
int nbdt_ref_bn_relu_pool(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                          const float* beta, int32_t B, int32_t H, int32_t W, int32_t C, float* pooled, void* stream);
int nbdt_ref_stem_conv(const float* img, const float* w, int32_t B, int32_t H, int32_t W, int32_t cout_real,
                       int32_t cpad, int32_t stride, float* out, void* stream);
int nbdt_ref_stem_wgrad(const float* img, const float* gy, int32_t B, int32_t H, int32_t W, int32_t cout_real,
                        int32_t cpad, int32_t stride, float* dw, void* stream);
/* fp32-storage twins of the MBConv pieces (EfficientNet-B0; verification only, like everything in this block): same
 * arguments and meaning as nbdt_bn_act_apply / _pool / _bwd and nbdt_dwconv_fwd / _bwd_data / _bwd_weight.  The fused
 * forms of the product path have no twin: a depthwise forward leaves no statistics (nbdt_ref_bn_stats re-reads the
 * tensor), and the data gradient with BatchNorm-backward sums is nbdt_ref_dwconv_bwd_data followed by the full
 * nbdt_ref_bn_act_bwd.  Replaces, for verification, pytorchcv dwconv / BatchNorm2d + Swish / SEBlock scaling behind
 * nbdt/models/__init__.py:3. */
int nbdt_ref_bn_act_apply(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                          const float* beta, int32_t act, const float* gate, const float* residual, int32_t B, int32_t H,
                          int32_t W, int32_t C, float* y, void* stream);
int nbdt_ref_bn_act_pool(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                         const float* beta, int32_t act, const float* mul, float scale, int32_t B, int32_t H, int32_t W,
                         int32_t C, float* out, void* stream);
int nbdt_ref_bn_act_bwd(const float* gu, const float* gate, const float* gpool, const float* x, const float* save_mean,
                        const float* save_rstd, const float* gamma, const float* beta, int32_t act, const float* gx_add,
                        int32_t B, int32_t H, int32_t W, int32_t C, float* dsum, float* dgamma, float* dbeta, float* gx,
                        void* stream);
/* twins of nbdt_bn_act_apply_rows / nbdt_bn_act_bwd_rows (stochastic depth): same arguments, meaning and refusals */
int nbdt_ref_bn_act_apply_rows(const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                               const float* beta, int32_t act, const float* gate, const float* residual,
                               const float* row_scale, int32_t B, int32_t H, int32_t W, int32_t C, float* y,
                               void* stream);
int nbdt_ref_bn_act_bwd_rows(const float* gu, const float* row_scale, const float* gate, const float* gpool,
                             const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
                             const float* beta, int32_t act, const float* gx_add, int32_t B, int32_t H, int32_t W,
                             int32_t C, float* dsum, float* dgamma, float* dbeta, float* gx, void* stream);
int nbdt_ref_dwconv_fwd(const float* x, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                        int32_t stride, float* y, void* stream);
int nbdt_ref_dwconv_bwd_data(const float* gy, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                             int32_t stride, float* gx, void* stream);
int nbdt_ref_dwconv_bwd_weight(const float* x, const float* gy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                               int32_t stride, float* dw, void* stream);

/* ------------------------------------------------------------------ stem / head / optimizer */
/* stem Conv2d(3->cout_real, 3x3, pad 1, stride 1|2) on NCHW fp32 images [B,3,H,W] -> padded NHWC
 * bf16 [B][H/stride+2][W/stride+2][cpad] (channels >= cout_real are zero).
 * w: fp32 [cout_real][3][3][3] (co, r, s, ci). */
int nbdt_stem_conv(const float* img, const float* w, int32_t B, int32_t H, int32_t W,
                   int32_t cout_real, int32_t cpad, int32_t stride, void* out, void* stream);
/* Weight gradient of that conv: dw[cout_real][3][3][3] (fp32) += sum over pixels of gy (padded NHWC bf16, channels
 * [0, cout_real)) x img.  cout_real must be a multiple of 8 and <= 72 (<= cpad): the kernel (round 4) reads the gradient
 * tile from LDS as float4 and keeps at most two 4-output groups per thread (every stem of the supported backbones is 16,
 * 32 or 64 wide).  Anything else returns NBDT_EINVAL -- rounds 1-3 accepted any cout_real <= 75. */
int nbdt_stem_wgrad(const float* img, const void* gy, int32_t B, int32_t H, int32_t W,
                    int32_t cout_real, int32_t cpad, int32_t stride, float* dw, void* stream);
/* nn.Linear: z[B][N] = x[B][K] w[N][K]^T + b (fp32) and its backward */
int nbdt_linear_fwd(const float* x, const float* w, const float* b, int32_t B, int32_t K, int32_t N,
                    float* z, void* stream);
int nbdt_linear_bwd(const float* x, const float* w, const float* gz, int32_t B, int32_t K, int32_t N,
                    float* gx, float* gw, float* gb, void* stream);
/* optim.SGD(momentum, weight_decay) over a flat fp32 buffer (main.py:207):
 * g = grad_scale*g + wd*p; buf = mom*buf + g; p -= lr*buf; optionally refreshes the bf16 copy the
 * conv kernels read (same element order as p) in the same pass; zero_grad != 0 also zeroes g (optimizer.zero_grad()
 * of the next step, main.py:235, folded into the same pass) */
int nbdt_sgd_step(float* p, float* g, float* buf, int64_t n, float lr, float momentum,
                  float weight_decay, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream);

/* ------------------------------------------------------------------ LARS (nbdt_version() >= 117) */
/* Layer-wise adaptive rate scaling (You et al. 2017; apex's LARC(clip=False) around optim.SGD) over the same three flat
 * fp32 buffers nbdt_sgd_step takes, for large global batches.  A plan holds a segment table of n_seg rows (offset, length,
 * weight_decay, adapt) over an arena of n elements: rows sorted by offset, disjoint, every offset a multiple of 4
 * elements, lengths arbitrary (>= 1).  Per segment s
 *   gn = sqrt(sum (grad_scale g_i)^2),  wn = sqrt(sum p_i^2),
 *   ratio_s = trust wn / (gn + wd_s wn + eps)  if adapt_s != 0 and wn > 0 and gn > 0, else 1
 * and per element of it
 *   u = ratio_s (grad_scale g_i + wd_s p_i);  buf_i = momentum buf_i + u;  p_i -= lr buf_i;  p_bf16_i = bf16(p_i)
 * -- optim.SGD(momentum, weight_decay=0) on the gradient ratio (g + wd p).  Elements outside every segment (alignment
 * gaps, the tail) are neither read for the norms nor written in p, buf or p_bf16; with zero_grad != 0 the whole of
 * g[0, n) is zero afterwards.  nbdt_lars_create checks the table (unsorted, overlapping, misaligned or out-of-range rows
 * and an empty table are NBDT_EINVAL before any device call), builds the wave -> (segment, range) tables on the host and
 * copies them, once, to the CURRENT device, with the workspace of the partial sums.  nbdt_lars_step is at most three
 * launches on `stream` (partial sums of squares, one fold per segment, the streaming update), no host synchronisation,
 * no floating-point atomics: which wave sums what, in which order, depends on the table alone, so a step is
 * bit-reproducible with nbdt_set_deterministic on or off.  p, g, buf: n fp32 elements each, 16-byte aligned; p_bf16: n
 * bf16 elements, 8-byte aligned, or NULL.  nbdt_lars_ratios: device pointer of ratio[n_seg] as the plan's last step left it
 * (1 before the first step), for tests and logging; owned by the plan. */
int nbdt_lars_create(int64_t n, const int64_t* offsets, const int64_t* lengths, const float* weight_decays,
                     const int32_t* adapt, int32_t n_seg, void** plan);
int nbdt_lars_destroy(void* plan);
int nbdt_lars_step(void* plan, float* p, float* g, float* buf, float lr, float momentum, float trust, float eps,
                   float grad_scale, void* p_bf16, int32_t zero_grad, void* stream);
const float* nbdt_lars_ratios(void* plan);
/* ... and a host copy of them: waits for `stream` (the one the step was issued on), then copies n_seg floats to out.
 * Synchronises the host: for tests and logging, never on the step path. */
int nbdt_lars_ratios_to_host(void* plan, float* out, void* stream);

/* ------------------------------------------------------------------ weight EMA (nbdt_version() >= 118) */
/* An exponential moving average of the weights (the `ModelEma` / `ExponentialMovingAverage` of the timm and torchvision
 * recipes) over the flat fp32 arena nbdt_sgd_step takes, and its in-place exchange with the live weights for evaluation.
 *   nbdt_ema_update:  per element  t = p - e;  e = e + one_minus_decay * t  -- three separately rounded fp32 operations (one
 *     subtract, one multiply, one add; never a fused multiply-add), the definition for every one_minus_decay in [0, 1], 0
 *     and 1 included.  One streaming pass over [0, n) with 16-byte accesses; p is only read.  Alignment gaps and padding
 *     that are zero in both buffers stay zero, so no segment table is taken.
 *   nbdt_ema_swap:    per element p and ema exchange values; with p_bf16 != NULL, p_bf16[i] = bf16(new p[i]), round to nearest
 *     even, what nbdt_sgd_step writes.  In place, because live tensors alias p: exchanging pointers would leave them behind.
 *   _multi: the same for n_rows small tensors in one launch (the BatchNorm running statistics).  `table` is a DEVICE array
 *     of n_rows rows (live pointer, shadow pointer, length) as int64, built once by the caller: pointers 16-byte
 *     aligned, lengths positive multiples of 32 elements, no tensor in two rows.  The rows cannot be checked on the host.
 * One launch each on `stream`, no host synchronisation, no atomics, nothing crosses a block: bit-reproducible by
 * construction.  Checked on the host before any device call (NBDT_EINVAL): NULL pointers, n <= 0 or n % 4 != 0, p / ema not
 * 16-byte aligned (p_bf16: 8-byte), p == ema, n_rows <= 0, one_minus_decay outside [0, 1] or NaN. */
int nbdt_ema_update(const float* p, float* ema, int64_t n, float one_minus_decay, void* stream);
int nbdt_ema_update_multi(const int64_t* table, int32_t n_rows, float one_minus_decay, void* stream);
int nbdt_ema_swap(float* p, float* ema, void* p_bf16, int64_t n, void* stream);
int nbdt_ema_swap_multi(const int64_t* table, int32_t n_rows, void* stream);

/* ------------------------------------------------------------------ AdamW and RMSprop (nbdt_version() >= 120) */
/* The adaptive optimizers over the flat fp32 arena nbdt_sgd_step takes, with a second state arena.  A plan holds the
 * segment table LARS takes without its adapt column: n_seg rows (offset, length, weight_decay) over n elements, sorted by
 * offset, disjoint, every offset a multiple of 4 elements, lengths arbitrary (>= 1).  nbdt_arena_opt_create checks the
 * table (an empty, unsorted, overlapping, misaligned or out-of-range one is NBDT_EINVAL before any device call), cuts
 * every segment into wave items of at most 512 elements, makes the gaps between segments and the tail items that only
 * zero g, and copies the item table, once, to the CURRENT device.  A step is ONE launch on `stream`, one wave per item,
 * 16-byte accesses with a scalar tail for length % 4, no atomics, no host synchronisation, nothing crosses a lane: it is
 * bit-reproducible with nbdt_set_deterministic on or off, and its result does not depend on where the items are cut.
 * Elements outside every segment are never written in p, the two state arenas or p_bf16; with zero_grad != 0 the whole of
 * g[0, n) is zero afterwards, else g is untouched.  p, g and the state arenas: n fp32 elements each (the plan's n),
 * 16-byte aligned; p_bf16: n bf16 elements, 8-byte aligned, or NULL.
 *
 * Every element update is the sequence of single IEEE fp32 operations below: each product, sum, difference, quotient and
 * square root is rounded once, to nearest even, in the order the parentheses give; nothing is fused, divisions and
 * square roots are correctly rounded.  fl(x) is x rounded to fp32.  The float arguments are fp32 values already; the
 * derived host scalars are formed in double from them and rounded ONCE:
 *   omb1 = fl(1 - (double)beta1), omb2 = fl(1 - (double)beta2), oma = fl(1 - (double)alpha),
 *   ss = fl((double)lr / (1 - pow((double)beta1, (double)t))),  c2 = fl(sqrt(1 - pow((double)beta2, (double)t))).
 * gs = grad_scale * g_i, wd the decay of the element's segment.
 *
 * nbdt_adamw_step -- torch.optim.AdamW (decoupled decay, no amsgrad), t >= 1 the number of this step:
 *   k = 1 - (lr * wd)                          (per segment, two fp32 operations)
 *   p1 = p * k
 *   m = (beta1 * m) + (omb1 * gs)
 *   v = (beta2 * v) + ((omb2 * gs) * gs)
 *   d = (sqrt(v) / c2) + eps
 *   p = p1 - (ss * (m / d));   p_bf16 = bf16(p)
 * nbdt_rmsprop_step, tf == 0 -- torch.optim.RMSprop (not centered):
 *   gs = gs + (wd * p)
 *   sq = (alpha * sq) + ((oma * gs) * gs)
 *   a = sqrt(sq) + eps
 *   momentum > 0:   buf = (momentum * buf) + (gs / a);   p = p - (lr * buf)
 *   momentum == 0:  p = p - (lr * (gs / a));  buf is neither read nor written and may be NULL
 * nbdt_rmsprop_step, tf != 0 -- TensorFlow's RMSprop, the one EfficientNet was trained with (epsilon inside the root, the
 * learning rate inside the momentum buffer; the caller starts sq at 1 inside the segments):
 *   gs = gs + (wd * p)
 *   sq = sq + (oma * ((gs * gs) - sq))
 *   a = sqrt(sq + eps)
 *   buf = (momentum * buf) + (lr * (gs / a));   p = p - buf
 * Checked on the host before any device call, in this order (NBDT_EINVAL): t < 1; beta1, beta2, alpha or momentum outside
 * [0, 1) or NaN; eps < 0 or NaN; lr or grad_scale not finite; a NULL plan; NULL or misaligned pointers; one buffer passed twice.  The plan's n
 * is the length of every buffer: the caller checks it (ops.ArenaOptPlan does). */
int nbdt_arena_opt_create(int64_t n, const int64_t* offsets, const int64_t* lengths, const float* weight_decays,
                          int32_t n_seg, void** plan);
int nbdt_arena_opt_destroy(void* plan);
int64_t nbdt_arena_opt_n(void* plan);            /* the n the plan was made for (0 for a NULL plan) */
int nbdt_adamw_step(void* plan, float* p, float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                    int64_t t, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream);
int nbdt_rmsprop_step(void* plan, float* p, float* g, float* sq, float* buf, float lr, float alpha, float eps,
                      float momentum, int32_t tf, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream);

/* ------------------------------------------------------------------ gradient clipping (nbdt_version() >= 121) */
/* Clipping by the global norm (torch.nn.utils.clip_grad_norm_, norm_type 2) over the flat fp32 gradient arena
 * nbdt_sgd_step takes, without a host read-back.  A plan holds the arena length n, a workspace of fp64 partial sums and a
 * 32-byte device record, on the CURRENT device.  Every operation below is ONE IEEE operation, rounded to nearest even.
 *
 * nbdt_clip_norm, two launches on `stream`:
 *   S = sum_{i<n} (double)g[i] * (double)g[i] over the whole arena g[0, n), in fp64 (each product of two floats is exact
 *   there).  The partition is fixed by n alone: B = min(2048, max(1, ceil(floor(n / 4) / 1024))) blocks of 256 threads,
 *   block b owning the 16-byte groups [b c, min((b + 1) c, floor(n / 4))), c = ceil(floor(n / 4) / B); thread t adds the
 *   groups t, t + 256, ... of its block's chunk into one fp64 accumulator per component (x, y, z, w), combines them as
 *   (x + y) + (z + w), and in the last block the threads t < n % 4 add element 4 floor(n / 4) + t; waves fold with the xor
 *   butterfly (offsets 32, 16, ..., 1), the four wave sums are added as ((w0 + w1) + w2) + w3, and one fp64 partial per
 *   block goes to the workspace.  The second launch is ONE block: thread t adds partials t, t + 256, ... in increasing
 *   index, then the same butterfly and wave-order sum.  No floating-point atomics, no last-block-done counter: the same g
 *   gives the same bits on every run, with nbdt_set_deterministic on or off.  Padding inside arena entries and the
 *   alignment gaps hold +0 in g (ParamStore.segments), so S is the sum over the logical parameters.  Then, in fp32,
 *     s32 = (float)S;  r = sqrtf(s32);  norm = fabsf(grad_scale) * r;  den = norm + 1e-6f;  coef = max_norm / den
 *   -- with grad_scale == 1, clip_grad_norm_'s coefficient -- and the record
 *     { float norm; float coef; int32 clipped; int32 steps; int32 nonfinite; int32 total_clipped; 8 bytes reserved }
 *   is updated by the one thread that writes it: steps += 1 on every call; norm not finite (inf or NaN): coef = 1,
 *   clipped = 0, nonfinite += 1; else coef < 1: clipped = 1, total_clipped += 1; else coef = 1, clipped = 0.  A new plan's
 *   record is {0, 1, 0, 0, 0, 0}.
 * nbdt_clip_apply, one launch on `stream`, the partition above: every wave reads coef from the record; coef == 1.0f: it
 *   returns before it touches g (an unclipped step costs one near-empty launch and no traffic); else g[i] = g[i] * coef,
 *   one fp32 multiply per element, 16-byte accesses and the scalar tail.  Elements at and beyond n are never written.
 * nbdt_clip_record: device pointer of the record, owned by the plan.  nbdt_clip_record_to_host: waits for `stream` (the
 *   one the launches were issued on), then copies the 32 bytes to out32.  Synchronises the host: for logging and tests,
 *   never on the step path.
 * Checked on the host before any device call, in this order (NBDT_EINVAL): max_norm not finite or <= 0; grad_scale not
 * finite; g NULL; g not 16-byte aligned; a NULL plan.  nbdt_clip_create: a NULL plan pointer, n <= 0.  g holds the plan's
 * n elements: the caller checks it (ops.ClipPlan does). */
int nbdt_clip_create(int64_t n, void** plan);
int nbdt_clip_destroy(void* plan);
int nbdt_clip_norm(void* plan, const float* g, float grad_scale, float max_norm, void* stream);
int nbdt_clip_apply(void* plan, float* g, void* stream);
const void* nbdt_clip_record(void* plan);
int nbdt_clip_record_to_host(void* plan, void* out32, void* stream);

/* ------------------------------------------------------------------ device-resident datasets (nbdt_version() >= 110) */
/* One launch builds a training batch from a dataset that lives in device memory: gather by index, then the reference's
 * RandomCrop(size, padding) -> RandomHorizontalFlip -> ToTensor -> Normalize (nbdt/data/cifar.py:11-21 pads CIFAR by 4,
 * nbdt/data/imagenet.py:37-48 pads TinyImagenet200 by 8), written as the fp32 NCHW tensor nbdt_stem_conv reads, with the
 * gathered targets.  csrc/augment.hip.
 *
 * Inputs
 *   src         the dataset [N,3,H,W] (NCHW), uint8 (src_dtype = NBDT_U8) or fp32 (NBDT_F32)
 *   labels_src  int64 [N]
 *   index       int64 [B], device memory: the samples of the batch, repeats allowed
 *   B, N, H, W  B > 0, N > 0, 1 <= H, W <= 4096; the crop size is always H x W, as in the reference
 *   pad         0 .. NBDT_AUGMENT_MAX_PAD pixels of padding on every side before the crop
 *   flip        0 | 1: enables the random horizontal flip of the generator
 *   mean, std   HOST float[3], copied into the kernel's arguments; uint8 sources only (may be NULL for fp32); std != 0
 *   fill        HOST float[3], the value of a padded pixel; fp32 sources only (may be NULL for uint8)
 *   seed, epoch the generator's key
 *   params_in   optional int8 [B,3] (dy, dx, flip), device memory: when non-NULL it REPLACES the generator (and `flip`).
 *               The entry validates every host-known argument; these values are device data, so the kernel clamps dy and
 *               dx to [0, 2*pad] and takes flip as (value != 0): a bad value can never index out of bounds.
 * Outputs
 *   out         fp32 [B,3,H,W]
 *   labels_out  int64 [B]
 *   params_out  optional int8 [B,3]: the (dy, dx, flip) actually used
 *
 * Semantics (crop, then flip: torchvision's order).  Output pixel (c, y, x) reads source (c, y + dy - pad, xs + dx - pad)
 * with xs = W-1-x when the sample is flipped, else x; dy, dx in [0, 2*pad].
 *   uint8:  value = ((float)u / 255.0f - mean[c]) / std[c] with u = 0 outside the image: the image is padded with byte 0
 *           BEFORE conversion, so a padded pixel is (0 - mean)/std, not 0.  Three IEEE fp32 operations in this order,
 *           no contraction, correctly rounded divisions: the bits of torch's CPU x.float().div(255).sub(mean).div(std).
 *   fp32:   the value is copied; outside the image it is fill[c].
 * pad = 0, flip = 0 is the evaluation transform: a plain gather + normalise.
 *
 * Out-of-range indices.  index is device data and cannot be checked on the host.  A sample whose index is outside [0, N)
 * is written as an all-zero image with label -1 and params (0, 0, 0); no address is formed from it.  (The loss kernels
 * answer a label outside [0, C) with a NaN loss, so the wrong batch is loud.)
 *
 * The draw is a pure function of (seed, epoch, dataset index, pad) -- not of the position in the batch, the batch size or
 * the rank -- so a batch is the concatenation of its halves and a sample gets the same crop in a 1-GPU and an 8-GPU run:
 *   mix64(x): x = (x ^ x>>30) * 0xBF58476D1CE4E5B9;  x = (x ^ x>>27) * 0x94D049BB133111EB;  return x ^ x>>31   (mod 2^64)
 *   key = mix64(seed * 0x9E3779B97F4A7C15 + epoch)
 *   r   = mix64(key ^ (index * 0xD1342543DE82EF95))
 *   dy  = ((r & 0xFFFFFF) * (2*pad+1)) >> 24;  dx = (((r >> 24) & 0xFFFFFF) * (2*pad+1)) >> 24;  flip = r >> 63
 * (nbdt/data.py draw_params restates it on the host.)  Replaces the DataLoader + torchvision transforms of reference
 * main.py:100-141. */
#define NBDT_U8 3                  /* src_dtype: uint8 (NBDT_F32 for fp32) */
#define NBDT_AUGMENT_MAX_PAD 32
int nbdt_augment_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int32_t B,
                       int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                       const float* fill, uint64_t seed, uint64_t epoch, const int8_t* params_in, float* out,
                       int64_t* labels_out, int8_t* params_out, void* stream);

/* ------------------------------------------------------------------ resized-crop datasets (nbdt_version() >= 111) */
/* The ImageNet transform family, one launch per batch from a uint8 dataset in device memory: gather by index, then
 * RandomResizedCrop(size) -> RandomHorizontalFlip -> ToTensor -> Normalize (training) or Resize(size + 32) ->
 * CenterCrop(size) -> ToTensor -> Normalize (evaluation), written as the fp32 NCHW tensor nbdt_stem_conv reads, with the
 * gathered targets.  Replaces the transforms of reference nbdt/data/imagenet.py:152-172.  csrc/resample.hip.
 *
 * Inputs
 *   src         the dataset [N,3,H,W] (NCHW), uint8: src_dtype must be NBDT_U8 (fp32 sources are refused, NBDT_EINVAL)
 *   labels_src  int64 [N]
 *   index       int64 [B], device memory, repeats allowed;  1 <= B <= 65535
 *   N, H, W     N > 0, 1 <= H, W <= 4096
 *   rs_h, rs_w  every sample's crop box is resampled to rs_h x rs_w (1..4096) ...
 *   win_top, win_left, out_h, out_w
 *               ... and only this window of the resampled image is computed and written.  Training: rs = out = size,
 *               window at (0, 0).  Evaluation: box = the whole image, rs = the image with its short side at size + 32
 *               (the long side int(short' * long / short), torchvision's Resize), window = the central size x size:
 *               Resize + CenterCrop without the discarded border.
 *   flip        0 | 1: enables the random horizontal flip of the generator
 *   mean, std   HOST float[3], std != 0
 *   scale, ratio  HOST double[2] each: the area-fraction range (0 < lo <= hi <= 1) and the aspect-ratio range
 *               (1/64 <= lo <= hi <= 64) of the draw; may be NULL with params_in
 *   ratio_table double [NBDT_RESIZED_CROP_RATIOS], DEVICE memory: the aspect ratios the draw chooses from, increasing from
 *               ratio[0] to ratio[1] (the caller fills it, in fp64, with exp(linspace(log lo, log hi, 4096))); may be NULL
 *               with params_in
 *   seed, epoch the generator's key
 *   params_in   optional int32 [B,5] (top, left, h, w, flip), device memory: when non-NULL it REPLACES the generator.
 *               Device data, so the kernel clamps: top to [0, H-1], left to [0, W-1], h to [1, H-top], w to [1, W-left],
 *               flip is (value != 0); a bad value can never index out of bounds.
 * Outputs
 *   out         fp32 [B,3,out_h,out_w]
 *   labels_out  int64 [B]
 *   params_out  optional int32 [B,5]: the (top, left, h, w, flip) actually used
 *
 * Resampling: PIL's BILINEAR as Image.resize applies it to an 8-bit image that was cropped to the box first.  Per axis,
 * for a box side `in` resampled to `out`: scale = in / out, support = max(1, scale), and output pixel i takes the taps
 * [xmin, xmax) with center = (i + 0.5) * scale, xmin = max(0, trunc(center - support + 0.5)),
 * xmax = min(in, trunc(center + support + 0.5)), weight(x) = max(0, 1 - |x - center + 0.5| / support), all in fp64; the
 * weights are divided by their sum and rounded to fixed point, k = trunc(0.5 + weight * 2^22).  The horizontal pass is
 * u8 = clip((2^21 + sum k * src) >> 22) to [0, 255]; the vertical pass does the same over those bytes.  Pure integer
 * arithmetic on fp64 coefficients: the result is PIL's, byte for byte (nbdt/data.py resample_reference restates it).
 * Then crop, then flip (output x reads resampled column out_w-1-x), then value = ((float)u8 / 255.0f - mean[c]) / std[c]:
 * the three IEEE fp32 operations of nbdt_augment_batch.
 *
 * The draw is torchvision's RandomResizedCrop.get_params, a pure function of (seed, epoch, dataset index) -- not of the
 * position in the batch, the batch size or the rank.  With mix64 and key as for nbdt_augment_batch and
 * G = 0x9E3779B97F4A7C15:
 *   base = mix64(key ^ (index * 0xD1342543DE82EF95));  flip = base >> 63
 *   attempt t = 0 .. NBDT_RESIZED_CROP_ATTEMPTS-1:  ra = mix64(base + (2t+1) * G);  rb = mix64(base + (2t+2) * G)
 *     target = (double)(H*W) * (scale[0] + (ra >> 11) * 2^-53 * (scale[1] - scale[0]))
 *     r      = ratio_table[rb & (NBDT_RESIZED_CROP_RATIOS-1)]
 *     w = round(sqrt(target * r));  h = round(sqrt(target / r))         (round half to even of the exact square root)
 *     accepted when 0 < w <= W and 0 < h <= H:  top = (((rb >> 12) & 0xFFFFFF) * (H-h+1)) >> 24,
 *                                               left = (((rb >> 36) & 0xFFFFFF) * (W-w+1)) >> 24
 *   no attempt accepted: the whole image, or with W/H < ratio[0]: h = round(W / ratio[0]); with W/H > ratio[1]:
 *   w = round(H * ratio[1]); centred.
 * Only fp64 multiply, divide, square root and rounding, one IEEE operation each, so nbdt/data.py
 * draw_resized_crop_params returns exactly these boxes.  The table quantises torchvision's log-uniform ratio to 4096
 * values: exp() is not correctly rounded on either side.
 *
 * Out-of-range indices: as for nbdt_augment_batch, a zero image with label -1 and params (0, 0, 0, 0, 0). */
#define NBDT_RESIZED_CROP_RATIOS 4096
#define NBDT_RESIZED_CROP_ATTEMPTS 10
int nbdt_resized_crop_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int32_t B,
                            int64_t N, int32_t H, int32_t W, int32_t rs_h, int32_t rs_w, int32_t win_top, int32_t win_left,
                            int32_t out_h, int32_t out_w, int32_t flip, const float* mean, const float* std,
                            const double* scale, const double* ratio, const double* ratio_table, uint64_t seed,
                            uint64_t epoch, const int32_t* params_in, float* out, int64_t* labels_out, int32_t* params_out,
                            void* stream);
/* Host only: the number of output rows one block of nbdt_resized_crop_batch computes for this geometry, with the source
 * rows of the band staged in LDS (16, 8, 4, 2 or 1: the largest whose worst-case tile fits 64 KB); 0 when no band fits and
 * the launch reads every source byte from global memory instead (same result, slower); -1 for a geometry the entry
 * refuses. */
int nbdt_resized_crop_band_rows(int32_t H, int32_t W, int32_t rs_h, int32_t rs_w, int32_t win_top, int32_t win_left,
                                int32_t out_h, int32_t out_w);

/* ------------------------------------------------------------------ rank-sharded datasets (nbdt_version() >= 114) */
/* nbdt_augment_batch / nbdt_resized_crop_batch for a rank that keeps only its contiguous part of the dataset: src and
 * labels_src hold the N samples [index_base, index_base + N) of a larger dataset, and index[] still holds indices into
 * that larger dataset.  Every other argument, every output and the arithmetic are those of the unsharded entry.
 *
 *   draw    from index[i] itself: the crop / flip / box of a sample stays a pure function of (seed, epoch, dataset index),
 *           whichever rank holds the sample and however many ranks there are
 *   gather  image row and label at index[i] - index_base
 *
 * index_base >= 0 and index_base + N must fit int64 (NBDT_EINVAL otherwise).  The unsharded entries ARE these with
 * index_base = 0: one kernel per family, the same bits.
 *
 * Out-of-range indices.  index is device data.  The kernel forms index[i] - index_base mod 2^64 and compares it unsigned
 * with N, so an index outside [index_base, index_base + N) -- another rank's sample, a negative value, anything -- never
 * becomes an address: the sample is written as an all-zero image with label -1 and zero params, as in the unsharded
 * entries.  nbdt/data.py refuses such an index on the host (ValueError) whenever the index tensor is host data. */
int nbdt_augment_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                               int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip,
                               const float* mean, const float* std, const float* fill, uint64_t seed, uint64_t epoch,
                               const int8_t* params_in, float* out, int64_t* labels_out, int8_t* params_out, void* stream);
int nbdt_resized_crop_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                    int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t rs_h,
                                    int32_t rs_w, int32_t win_top, int32_t win_left, int32_t out_h, int32_t out_w,
                                    int32_t flip, const float* mean, const float* std, const double* scale,
                                    const double* ratio, const double* ratio_table, uint64_t seed, uint64_t epoch,
                                    const int32_t* params_in, float* out, int64_t* labels_out, int32_t* params_out,
                                    void* stream);

/* ------------------------------------------------------------------ ImageNet-style stem (nbdt_version() >= 115) */
/* The front of torchvision's ResNet -- Conv2d(3, 64, 7, stride 2, padding 3) -> BatchNorm -> ReLU -> MaxPool2d(3, 2, 1)
 * (reference nbdt/models/__init__.py takes these networks from torchvision.models) -- as two data-movement ops around the
 * launches above.  csrc/stem_pool.hip.  dtype: the storage of the padded NHWC tensors, NBDT_BF16 (product) or NBDT_F32 (the
 * engines' reference mode).  No atomics anywhere: the same inputs give the same bits.
 *
 * nbdt_stem_patches: img fp32 NCHW [B][3][H][W] -> out padded NHWC [B][H/stride+2][W/stride+2][cpad] with
 *   out[b][oy+1][ox+1][(r*k + s)*3 + ci] = img[b][ci][oy*stride - k/2 + r][ox*stride - k/2 + s]   (0 outside the image)
 * and zeros in channels [3*k*k, cpad), converted with round-to-nearest-even for bf16.  A k x k / stride / padding k/2
 * convolution of the image is then the 1x1 convolution of `out` with w[cout][1][cpad] (nbdt_conv_igemm[_stats|_affine]), and
 * its weight gradient is nbdt_conv_wgrad's.  Only interior pixels are written (the ring is left as it is).  k odd and <= 7,
 * stride 1 or 2, H and W divisible by stride, cpad a multiple of 32 with cpad >= 3*k*k; anything else is NBDT_EINVAL. */
int nbdt_stem_patches(const float* img, int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t cpad,
                      int32_t dtype, void* out, void* stream);
/* MaxPool2d(kernel_size=3, stride=2, padding=1): x padded NHWC [B][H+2][W+2][C] -> y [B][H/2+2][W/2+2][C], interior pixels
 * only.  torch's semantics: positions outside the image do not take part (decided by their indices; the ring is never
 * read), the winner is the first maximum in row-major window order, NaN propagates.  idx (NULL in inference): uint8
 * [B][H/2][W/2][C], the winner's window position 3*dy + dx relative to the window origin (2*oy - 1, 2*ox - 1).
 * H and W even, C a multiple of 8. */
int nbdt_maxpool3x3s2_fwd(const void* x, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, void* y, uint8_t* idx,
                          void* stream);
/* Its backward as a gather: gx[b][y][x][c] = the fp32 sum, rounded once, of gy over the (at most 2 x 2) windows that contain
 * (y, x) and whose idx names it -- zero where none does.  Every interior element of gx is written with a plain store. */
int nbdt_maxpool3x3s2_bwd(const void* gy, const uint8_t* idx, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                          void* gx, void* stream);

/* ------------------------------------------------------------------ batch mixing (nbdt_version() >= 116) */
/* MixUp / CutMix of a training batch with itself rolled by one (torchvision v2's pairing: the partner of sample b is
 * (b - 1) mod B), and the probability targets that go with it, in ONE streaming launch.  csrc/mix.hip.
 *   x    fp32 [B][3][H][W];  y int64 [B], device memory;  out fp32 [B][3][H][W], must not overlap x (NBDT_EINVAL)
 *   out  = x*lam + x_partner*one_minus_lam outside the box (two fp32 multiplies and one add, no contraction: the bits of
 *          torch's x.mul(lam).add(x.roll(1, 0).mul(one_minus_lam))), and x_partner inside the box [y1, y2) x [x1, x2).
 *          MixUp: an empty box (y1 == y2 or x1 == x2).  CutMix: lam = 1, one_minus_lam = 0 and a box;
 *          0 <= y1 <= y2 <= H, 0 <= x1 <= x2 <= W.  With lam = 1 and one_minus_lam = 0 the element outside the box is x
 *          itself, copied (CutMix's semantics): for MixUp at exactly lam = 1 that is torch's x*1 + x_partner*0 only where
 *          x_partner is finite (an inf / NaN partner pixel gives NaN there, x here).
 *   tgt  fp32 [B][C], must not overlap x or out (NBDT_EINVAL), every element written:  tgt[b] = onehot(y_b)*lam_t + onehot(y_partner)*one_minus_lam_t.
 * A label outside [0, C) (the -1 of a sample a shard does not hold) gives an all-NaN target row, which the loss kernels
 * turn into a NaN loss; no address is formed from it.  16-byte accesses when W % 4 == 0 and the pointers are 16-byte
 * aligned, scalar otherwise.  No atomics: the same inputs give the same bits. */
int nbdt_mix_batch(const float* x, const int64_t* y, int32_t B, int32_t H, int32_t W, float lam, float one_minus_lam,
                   int32_t y1, int32_t y2, int32_t x1, int32_t x2, float lam_t, float one_minus_lam_t, float* out,
                   float* tgt, int32_t C, void* stream);

/* ------------------------------------------------------------------ augmentation policy (nbdt_version() >= 119) */
/* nbdt_augment_batch with an augmentation policy, still ONE launch per batch: gather by index, zero-padded random crop,
 * flip, then ONE TrivialAugmentWide operation on the uint8 image, then /255 and Normalize, then torchvision's
 * RandomErasing(value=0) on the normalised output.  csrc/policy.hip, policy_kernel: its own single-operation kernel, on the
 * draw, statistics and output functions of the chain kernel below.  The recipe of the TrivialAugment paper's CIFAR setup
 * and of torchvision's ResNet reference (ta_wide, RandomErasing(0.1)).  nbdt_policy_batch_sharded is the entry for a rank
 * that holds the samples [index_base, index_base + N) (see nbdt_augment_batch_sharded); nbdt_policy_batch is its base-0 form.
 *
 * src, src_dtype, labels_src, index, B, N, H, W, pad, flip, mean, std, seed, epoch, params_in, out, labels_out, params_out:
 * as for nbdt_augment_batch, except that src_dtype must be NBDT_U8 and 3*H*W at most 49152 bytes (the image is staged in
 * LDS twice); anything else is NBDT_EINVAL.  The crop / flip draw is nbdt_augment_batch's: a sample gets the same crop with
 * and without the policy.  Further arguments:
 *   policy        NBDT_POLICY_NONE (every sample gets Identity) | NBDT_POLICY_TA_WIDE
 *   policy_table  int32 [NBDT_POLICY_OPS][NBDT_POLICY_BINS][2][6], DEVICE memory; needed unless policy is NBDT_POLICY_NONE
 *                 and policy_in is NULL.  Per (op, bin, sign) the magnitude in the form the kernel consumes, formed by the
 *                 caller in fp64 (nbdt/data.py policy_table), so that the device does no trigonometry:
 *                   ShearX/Y, TranslateX/Y, Rotate   Pillow's 16.16 fixed-point affine coefficients a0 .. a5 (below)
 *                   Brightness, Color, Contrast, Sharpness   word 0 = the bits of (float)factor
 *                   Posterize  word 0 = the byte mask;   Solarize  word 0 = ceil(threshold);   other words 0
 *   erase_prob    in [0, 1]: the probability that a sample is erased
 *   erase_scale, erase_ratio  HOST double[2] each, as scale / ratio of nbdt_resized_crop_batch (torchvision's defaults are
 *                 (0.02, 0.33) and (0.3, 3.3)); ratio_table: the NBDT_RESIZED_CROP_RATIOS log-spaced ratios, DEVICE memory.
 *                 All three are needed only when erase_prob > 0 and policy_in is NULL.
 *   policy_in     optional int32 [B,7] (op, bin, sign, top, left, h, w), device memory: REPLACES the policy and erase draw.
 *                 Device data, so the kernel clamps: op to [0, 13], bin to [0, 30], sign is (value != 0), top to [0, H-1],
 *                 left to [0, W-1], h to [0, H-top], w to [0, W-left]; h == 0 or w == 0 erases nothing.
 *   policy_out    optional int32 [B,7]: the values actually used (an empty rectangle is reported as 0, 0, 0, 0)
 *
 * The operations, in the kernel's order (op = 0 .. 13), for bin b in 0 .. 30 and s = +1 (sign 0) or -1 (sign 1); the
 * magnitudes are TrivialAugmentWide's, the pixel rules are Pillow's (what torchvision calls on PIL images), fill = byte 0:
 *   Identity
 *   ShearX, ShearY      m = s*0.99*b/30; Image.transform(AFFINE, NEAREST) with [1, m, 0, 0, 1, 0] / [1, 0, 0, m, 1, 0]
 *   TranslateX, TranslateY   t = s*int(32*b/30) pixels: source x - t / y - t
 *   Rotate              Image.rotate(s*135*b/30 degrees, NEAREST): centre (W/2, H/2), matrix entries round(cos, 15) and
 *                       round(sin, 15) of -radians(angle % 360); angle 0 is a copy and +-90 on a square image the exact
 *                       transpose (Pillow's special cases)
 *   Brightness, Color, Contrast, Sharpness   ImageEnhance: blend(degenerate, image, 1 + s*0.99*b/30); the degenerate image
 *                       is black / the grey image / the solid grey mean int(mean(grey) + 0.5) / ImageFilter.SMOOTH
 *                       ((1 1 1; 1 5 1; 1 1 1)/13 as trunc(sum/13 + 0.5), the one-pixel border copied);
 *                       grey = (19595 R + 38470 G + 7471 B + 32768) >> 16;  blend in fp32: t = d + a*(x - d), a separate
 *                       multiply and add, then 0 for t <= 0, 255 for t >= 255, else truncated
 *   Posterize           v & ~(2^(8-bits) - 1), bits = 8 - round(b/5)
 *   Solarize            v if v < 255 - 255*b/30 else 255 - v
 *   AutoContrast        ImageOps.autocontrast, per channel: lo, hi = min, max; unchanged if hi <= lo, else
 *                       clip(int(v*scale + offset)) with scale = 255.0/(hi - lo), offset = -lo*scale in fp64
 *   Equalize            ImageOps.equalize, per channel: histogram h; unchanged with at most one non-empty bin or
 *                       step = (H*W - h[last non-empty]) / 255 == 0; else lut[i] = min(255, (step/2 + sum h[j<i]) / step)
 * Nearest affine (Pillow's affine_fixed): output pixel (x, y) reads source ((a2 + a0*x + a1*y) >> 16,
 * (a5 + a3*x + a4*y) >> 16) when that lies inside the image, else 0, with FIX(v) = floor-for-negative int(v*65536 + 0.5),
 * a0, a1, a3, a4 = FIX of the matrix entries, a2 = FIX(m[2] + 0.5*m[0] + 0.5*m[1]), a5 = FIX(m[5] + 0.5*m[3] + 0.5*m[4]).
 * Parity with torchvision's own float32 linspace magnitudes and its atan/tan shear round trip is NOT claimed.
 *
 * The draw.  With mix64 and key as for nbdt_augment_batch and G = 0x9E3779B97F4A7C15:
 *   rp = mix64(key ^ (index * 0xA0761D6478BD642F)):   op = ((rp & 0xFFFFFF) * 14) >> 24;
 *                                                      bin = (((rp >> 24) & 0xFFFFFF) * 31) >> 24;  sign = rp >> 63
 *   re = mix64(key ^ (index * 0xE7037ED1A0B428DB)):   erased when (re >> 11) * 2^-53 < erase_prob; then
 *   attempt t = 0 .. NBDT_RESIZED_CROP_ATTEMPTS-1:  ra = mix64(re + (2t+1) * G);  rb = mix64(re + (2t+2) * G)
 *     target = (double)(H*W) * (scale[0] + (ra >> 11) * 2^-53 * (scale[1] - scale[0]))
 *     r = ratio_table[rb & (NBDT_RESIZED_CROP_RATIOS-1)];  h = round(sqrt(target * r));  w = round(sqrt(target / r))
 *     the first attempt with h < H and w < W is taken:  top = (((rb >> 12) & 0xFFFFFF) * (H-h+1)) >> 24,
 *                                                       left = (((rb >> 36) & 0xFFFFFF) * (W-w+1)) >> 24
 *   no such attempt: nothing is erased.
 * A pure function of (seed, epoch, dataset index) and the settings -- not of the position in the batch, the batch size or
 * the rank (nbdt/data.py draw_policy_params restates it).  Erased pixels are exactly 0.0f in the normalised output.
 *
 * The per-image statistics (grey sum, channel minima / maxima, histograms) are integer LDS atomics: the same inputs give
 * the same bits.  Out-of-range indices: a zero image with label -1 and zero params, as for nbdt_augment_batch. */
#define NBDT_POLICY_NONE 0
#define NBDT_POLICY_TA_WIDE 1
#define NBDT_POLICY_OPS 14
#define NBDT_POLICY_BINS 31
int nbdt_policy_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int32_t B,
                      int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                      int32_t policy, const int32_t* policy_table, double erase_prob, const double* erase_scale,
                      const double* erase_ratio, const double* ratio_table, uint64_t seed, uint64_t epoch,
                      const int8_t* params_in, const int32_t* policy_in, float* out, int64_t* labels_out,
                      int8_t* params_out, int32_t* policy_out, void* stream);
int nbdt_policy_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                              int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip,
                              const float* mean, const float* std, int32_t policy, const int32_t* policy_table,
                              double erase_prob, const double* erase_scale, const double* erase_ratio,
                              const double* ratio_table, uint64_t seed, uint64_t epoch, const int8_t* params_in,
                              const int32_t* policy_in, float* out, int64_t* labels_out, int8_t* params_out,
                              int32_t* policy_out, void* stream);

/* ------------------------------------------------------------------ policy chains (nbdt_version() >= 123) */
/* RandAugment and AutoAugment: nbdt_policy_batch with up to NBDT_CHAIN_MAX_OPS operations per image, still ONE launch per
 * batch (policy_chain_kernel, csrc/policy.hip).  Order: gather, zero-padded crop, flip, the chain on the bytes, /255 and
 * Normalize, erase.  After the crop the source tile is free, so the chain ping-pongs between the two LDS tiles: every
 * non-Identity slot but the last is one byte pass, the last one is evaluated inside the normalising output pass, the
 * per-image statistics (grey sum, minima / maxima, histograms) are collected again on the tile an operation reads.  An
 * Identity slot costs nothing.  The LDS budget, so the 3*H*W <= 49152 limit and the uint8-only source, are
 * nbdt_policy_batch's, and so are the arguments src .. std, erase_prob .. epoch, params_in, out, labels_out, params_out.
 *
 * Pixel rules: those of nbdt_policy_batch for op 0 .. 13, fill byte 0, plus op 14 = Invert (255 - v): NBDT_CHAIN_OPS = 15.
 * Magnitudes for a policy with n = nbins bins, bin b, s = +1 (sign 0) or -1 (sign 1), each formed in double as hi*b/(n-1)
 * (torchvision's _augmentation_space of RandAugment, n = 31, and of AutoAugment, n = 10; nbdt/data.py chain_table):
 *   ShearX, ShearY      m = s*0.3*b/(n-1)
 *   TranslateX          t = s*int((150/331)*W*b/(n-1)) pixels, source x - t;   TranslateY: the same with H
 *   Rotate              s*30*b/(n-1) degrees
 *   Brightness, Color, Contrast, Sharpness   factor 1 + s*0.9*b/(n-1)
 *   Posterize           bits = 8 - round(b / ((n-1)/4));   Solarize: threshold 255 - 255*b/(n-1)
 *   Identity, AutoContrast, Equalize, Invert   none
 * Pillow with these double magnitudes is the oracle; parity with torchvision's own float32 linspace magnitudes and its
 * atan/tan shear round trip is NOT claimed.
 *   mode          NBDT_CHAIN_RAND | NBDT_CHAIN_SUBPOLICY
 *   nbins         1 .. NBDT_CHAIN_MAX_BINS
 *   table         int32 [NBDT_CHAIN_OPS][nbins][2][6], DEVICE memory, rows in the form of policy_table
 *   num_ops, magnitude   NBDT_CHAIN_RAND: 1 .. NBDT_CHAIN_MAX_OPS slots, each at bin `magnitude` < nbins (ignored otherwise)
 *   subpolicies, P       NBDT_CHAIN_SUBPOLICY: int32 [P][NBDT_CHAIN_MAX_OPS][3] of (op, q = round(p * 2^24), bin), DEVICE
 *                 memory, P in 1 .. NBDT_CHAIN_MAX_SUBPOLICIES; an unused slot is op 0 / q 0.  The host reads nothing from it:
 *                 the kernel clamps op to [0, 14], q to [0, 2^24], bin to [0, nbins-1]
 *   chain_in      optional int32 [B][NBDT_CHAIN_MAX_OPS][3] (op, bin, sign), device memory: REPLACES the chain's draw; clamped
 *                 by the kernel: op to [0, 14], bin to [0, nbins-1], sign is (value != 0)
 *   erase_in      optional int32 [B][4] (top, left, h, w), device memory: REPLACES the erase draw; clamped as policy_in's
 *   chain_out, erase_out   optional, the values actually used; a skipped or unused slot is Identity (0, 0, 0)
 *
 * The draw.  The crop / flip word and the erase word `re` are nbdt_policy_batch's: a sample gets the same crop and the same
 * erase rectangle under every policy setting.  The chain adds, with mix64, key and G as above:
 *   rc = mix64(key ^ (index * 0x8EBC6AF09C88C6E3));   slot k = 0 .. 3:  rs = mix64(rc + (k+1) * G)
 *   NBDT_CHAIN_RAND, k < num_ops:   op = ((rs & 0xFFFFFF) * 14) >> 24 (Invert is not in its space);  bin = magnitude;
 *                                   sign = rs >> 63
 *   NBDT_CHAIN_SUBPOLICY:   the sub-policy is ((rc & 0xFFFFFF) * P) >> 24; its slot k = (op, q, bin) is applied when
 *                           (rs & 0xFFFFFF) < q (exact: p = 0 never, p = 1 always; it replaces torchvision's rand() <= p),
 *                           with sign = 1 - (rs >> 63) (negative magnitude when the sign bit is 0, torchvision's
 *                           signs[i] == 0); a slot that is not applied is Identity
 * A pure function of (seed, epoch, dataset index) and the settings (nbdt/data.py draw_chain_params restates it).
 * Integer statistics, as for nbdt_policy_batch: the same inputs give the same bits.  Out-of-range indices: a zero image,
 * label -1, zero params.  nbdt_policy_batch itself is unchanged and keeps refusing policy = 2. */
#define NBDT_CHAIN_OPS 15
#define NBDT_CHAIN_MAX_OPS 4
#define NBDT_CHAIN_MAX_BINS 31
#define NBDT_CHAIN_MAX_SUBPOLICIES 1024
#define NBDT_CHAIN_RAND 0
#define NBDT_CHAIN_SUBPOLICY 1
int nbdt_policy_chain_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int32_t B,
                            int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean,
                            const float* std, int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops,
                            int32_t magnitude, const int32_t* subpolicies, int32_t P, double erase_prob,
                            const double* erase_scale, const double* erase_ratio, const double* ratio_table, uint64_t seed,
                            uint64_t epoch, const int8_t* params_in, const int32_t* chain_in, const int32_t* erase_in,
                            float* out, int64_t* labels_out, int8_t* params_out, int32_t* chain_out, int32_t* erase_out,
                            void* stream);
int nbdt_policy_chain_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                    int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad,
                                    int32_t flip, const float* mean, const float* std, int32_t mode, int32_t nbins,
                                    const int32_t* table, int32_t num_ops, int32_t magnitude, const int32_t* subpolicies,
                                    int32_t P, double erase_prob, const double* erase_scale, const double* erase_ratio,
                                    const double* ratio_table, uint64_t seed, uint64_t epoch, const int8_t* params_in,
                                    const int32_t* chain_in, const int32_t* erase_in, float* out, int64_t* labels_out,
                                    int8_t* params_out, int32_t* chain_out, int32_t* erase_out, void* stream);

/* ------------------------------------------------------------------ resized-crop policy (nbdt_version() >= 124) */
/* The policy chains and the erase on the ImageNet-style path: gather, RandomResizedCrop(S), flip, a chain of up to
 * NBDT_CHAIN_MAX_OPS of the 15 operations on the S x S bytes, /255 and Normalize, RandomErasing(value=0), into out
 * [B,3,S,S] fp32.  torchvision's RandomResizedCrop -> RandomHorizontalFlip -> {TrivialAugmentWide | RandAugment |
 * AutoAugment} -> ToTensor -> Normalize -> RandomErasing, on the device with no host read-back (csrc/resample.hip).
 *
 * Two launches inside the one entry, both on `stream`.  (1) nbdt_resized_crop_batch's kernels in their byte-output mode:
 * the same boxes, the same resampling arithmetic, the resized and flipped uint8 image into stage_a; labels_out and
 * params_out as ever.  (2) One block per image applies the chain, ping-ponging between the image's 3*S*S bytes of stage_a
 * and of stage_b: a tile of 150 KB at S = 224 does not fit the LDS tiles of nbdt_policy_chain_batch (49152 bytes), so the
 * two tiles live in global memory, written and re-read by one block on one CU (its L1, its XCD's L2), ordered by workgroup
 * barriers; only the statistics (three histograms, grey sum, minima / maxima, AutoContrast's scale and offset) are in LDS.
 * As there: an Identity slot costs no pass, statistics are collected again on the tile an operation reads, the last
 * non-Identity operation is evaluated inside the normalising output pass, which also zeroes the erase rectangle.
 *
 * Pixel rules, magnitudes and draws are nbdt_policy_chain_batch's with H = W = S: `table` is built for the S x S crop
 * (translations (150/331) * S, Rotate about (S/2, S/2)), the erase rectangle is drawn in the S x S output, and every draw
 * hashes the GLOBAL dataset index, so a sample's box and flip are nbdt_resized_crop_batch's with and without a policy.
 *   src .. ratio_table   as nbdt_resized_crop_batch (rs_h = rs_w = out_h = out_w = S, window (0, 0): training only)
 *   S             1 .. NBDT_RESIZED_CROP_POLICY_MAX_SIDE.  Contrast's grey sum and its rounding (2*sum + S*S) / (2*S*S) are
 *                 formed in 32 bits: at 512^2 the largest intermediate is 2*255*262144 + 262144 ~ 1.3e8; at 4096^2 it
 *                 would overflow, so larger sides are refused
 *   mode          NBDT_CHAIN_RAND | NBDT_CHAIN_SUBPOLICY as above, num_ops 0 .. NBDT_CHAIN_MAX_OPS (0: no operation, the erase
 *                 only; `table` may then be NULL unless chain_in is given), or NBDT_CHAIN_TA_WIDE (this entry only): ONE slot
 *                 whose (op, bin, sign) is nbdt_policy_batch's draw -- rp = mix64(key ^ (index * 0xA0761D6478BD642F)),
 *                 op = ((rp & 0xFFFFFF) * 14) >> 24, bin = (((rp >> 24) & 0xFFFFFF) * 31) >> 24, sign = rp >> 63 -- on a table of
 *                 TrivialAugmentWide's ranges: nbins must be NBDT_POLICY_BINS
 *   nbins, table, num_ops, magnitude, subpolicies, P      as nbdt_policy_chain_batch
 *   erase_prob, erase_scale, erase_ratio, erase_ratio_table   as nbdt_policy_chain_batch's erase_prob .. ratio_table
 *   params_in / params_out   int32 [B][5] (top, left, h, w, flip) as nbdt_resized_crop_batch
 *   chain_in, erase_in, chain_out, erase_out   as nbdt_policy_chain_batch, clamped the same way (op to [0, 14], bin to
 *                 [0, nbins-1], sign != 0, the rectangle into the S x S output)
 *   stage_a, stage_b   uint8 [B][3][S][S] each, device memory, 16-byte aligned, distinct: scratch, contents undefined after
 * Every value read from device memory (index, params, chain slots, rectangles, sub-policy rows) is clamped or
 * bounds-checked before an address is formed from it.  Out-of-range indices (index < index_base or >= index_base + N,
 * compared unsigned): a zero image, label -1, zero params; no source address is formed.  Integer statistics: the same
 * inputs give the same bits. */
#define NBDT_CHAIN_TA_WIDE 2
#define NBDT_RESIZED_CROP_POLICY_MAX_SIDE 512
int nbdt_resized_crop_policy_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                   int32_t B, int64_t N, int32_t H, int32_t W, int32_t S, int32_t flip, const float* mean,
                                   const float* std, const double* scale, const double* ratio, const double* ratio_table,
                                   int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops, int32_t magnitude,
                                   const int32_t* subpolicies, int32_t P, double erase_prob, const double* erase_scale,
                                   const double* erase_ratio, const double* erase_ratio_table, uint64_t seed, uint64_t epoch,
                                   const int32_t* params_in, const int32_t* chain_in, const int32_t* erase_in, void* stage_a,
                                   void* stage_b, float* out, int64_t* labels_out, int32_t* params_out, int32_t* chain_out,
                                   int32_t* erase_out, void* stream);
int nbdt_resized_crop_policy_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                           const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                           int32_t W, int32_t S, int32_t flip, const float* mean, const float* std,
                                           const double* scale, const double* ratio, const double* ratio_table, int32_t mode,
                                           int32_t nbins, const int32_t* table, int32_t num_ops, int32_t magnitude,
                                           const int32_t* subpolicies, int32_t P, double erase_prob,
                                           const double* erase_scale, const double* erase_ratio,
                                           const double* erase_ratio_table, uint64_t seed, uint64_t epoch,
                                           const int32_t* params_in, const int32_t* chain_in, const int32_t* erase_in,
                                           void* stage_a, void* stage_b, float* out, int64_t* labels_out, int32_t* params_out,
                                           int32_t* chain_out, int32_t* erase_out, void* stream);

/* ------------------------------------------------------------------ padded strided convolutions (nbdt_version() >= 126)
 * The depthwise and stem convolutions for ANY extent and a low-side padding, per axis:
 *   Ho = ceil(H / stride);  output o reads inputs o * stride + r - pad_lo for r in [0, k);  reads outside [0, H) are zero.
 * pad_lo = k / 2 is PyTorch's symmetric padding=k/2 (for which the functions above are the special case "the stride
 * divides the extent"); TensorFlow's "SAME" padding is pad_lo = max((Ho - 1) * stride + k - H, 0) / 2, which differs from
 * it only at stride 2 on an even extent: 0 at k = 3, 1 at k = 5.  pad_top / pad_left are the two axes' pad_lo.
 * Tensors, weights, bn_scratch and deterministic mode as in nbdt_dwconv_fwd / _bwd_data / _bwd_weight and nbdt_stem_conv /
 * _wgrad, with y / gy of size [B][Ho + 2][Wo + 2][C]; with pad_lo = k / 2 on even extents the results are theirs bit for
 * bit.  NBDT_EINVAL before any device work: pad_top or pad_left outside [0, k / 2], k not 3 or 5 (the stem is k = 3),
 * stride not 1 or 2, stride 1 with a padding other than k / 2, non-positive extents. */
int nbdt_dwconv_fwd_pad(const void* x, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                        int32_t stride, int32_t pad_top, int32_t pad_left, void* y, float* bn_scratch, void* stream);
/* H, W: the INPUT-sized gradient being written */
int nbdt_dwconv_bwd_data_pad(const void* gy, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                             int32_t stride, int32_t pad_top, int32_t pad_left, void* gx, void* stream);
int nbdt_dwconv_bwd_weight_pad(const void* x, const void* gy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                               int32_t stride, int32_t pad_top, int32_t pad_left, float* dw, void* stream);
int nbdt_stem_conv_pad(const float* img, const float* w, int32_t B, int32_t H, int32_t W, int32_t cout_real, int32_t cpad,
                       int32_t stride, int32_t pad_top, int32_t pad_left, void* out, void* stream);
int nbdt_stem_wgrad_pad(const float* img, const void* gy, int32_t B, int32_t H, int32_t W, int32_t cout_real, int32_t cpad,
                        int32_t stride, int32_t pad_top, int32_t pad_left, float* dw, void* stream);
/* their fp32 twins (reference mode, see nbdt_ref_dwconv_fwd) */
int nbdt_ref_dwconv_fwd_pad(const float* x, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                            int32_t stride, int32_t pad_top, int32_t pad_left, float* y, void* stream);
int nbdt_ref_dwconv_bwd_data_pad(const float* gy, const float* w, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                                 int32_t stride, int32_t pad_top, int32_t pad_left, float* gx, void* stream);
int nbdt_ref_dwconv_bwd_weight_pad(const float* x, const float* gy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                                   int32_t stride, int32_t pad_top, int32_t pad_left, float* dw, void* stream);
int nbdt_ref_stem_conv_pad(const float* img, const float* w, int32_t B, int32_t H, int32_t W, int32_t cout_real,
                           int32_t cpad, int32_t stride, int32_t pad_top, int32_t pad_left, float* out, void* stream);
int nbdt_ref_stem_wgrad_pad(const float* img, const float* gy, int32_t B, int32_t H, int32_t W, int32_t cout_real,
                            int32_t cpad, int32_t stride, int32_t pad_top, int32_t pad_left, float* dw, void* stream);

/* ------------------------------------------------------------------ agglomerative clustering (nbdt_version() >= 128)
 * What scipy.cluster.hierarchy.linkage / sklearn's AgglomerativeClustering compute for an induced hierarchy, on the
 * device in fp64 (csrc/linkage.hip): one launch writes the full pairwise distance matrix of the n rows of `centers`
 * (fp32 [n][d], contiguous, device memory) into the workspace, a second one -- a single workgroup -- runs the
 * nearest-neighbour chain over it and writes the n - 1 merges in the order it found them:
 *   merges_out  int32 [n-1][2]   (retired index, kept index): the two clusters merged, smaller index first; the merged
 *                                cluster lives on under the larger index
 *   heights_out fp64  [n-1]      the linkage distance of the merge
 *   sizes_out   int32 [n-1]      leaves of the merged cluster (0 in every row of a run that did not finish, which only
 *                                NaN distances can cause)
 * Sorting the rows by height (stable) and relabelling with a union-find in which merge i creates cluster n + i gives
 * scipy's linkage matrix (nbdt.graph.linkage_children does that on the host).  Ties are resolved towards the previous
 * chain element, then the lowest index: same inputs, same bits.
 * The workspace holds the matrix (8 n^2 bytes) and two int32 [n] arrays (cluster sizes, the chain);
 * nbdt_linkage_workspace_bytes gives its size.  Its contents after a call are scratch, except that the first int32 of
 * the second array (byte offset 8 n^2 + 4 n) holds the number of chain steps taken, for profiles.
 * NBDT_EINVAL before any device call, outputs untouched: null pointers, n < 2 (or above 2^20), d < 1 (or above 2^24),
 * an unknown method or metric, ward with another metric than euclidean, a workspace smaller than that size, misaligned
 * pointers (8 bytes for workspace and heights_out, 4 for the others). */
#define NBDT_LINKAGE_WARD 0
#define NBDT_LINKAGE_COMPLETE 1
#define NBDT_LINKAGE_SINGLE 2
#define NBDT_LINKAGE_AVERAGE 3
#define NBDT_METRIC_EUCLIDEAN 0
#define NBDT_METRIC_MANHATTAN 1     /* sklearn's l1 / manhattan / cityblock */
#define NBDT_METRIC_COSINE 2        /* 1 - x.y / (|x| |y|), the cosine clipped to [-1, 1] as scipy's pdist does */
int nbdt_linkage_workspace_bytes(int64_t n, int64_t* bytes);
int nbdt_linkage(const float* centers, int64_t n, int64_t d, int32_t method, int32_t metric, void* workspace,
                 int64_t workspace_bytes, int32_t* merges_out, double* heights_out, int32_t* sizes_out, void* stream);

/* ------------------------------------------------------------------ measurement probe (not on the product path) */
/* A register-only stream of independent v_mfma_f32_32x32x16_bf16 on `blocks` CUs (one 512-thread block each, two waves
 * per SIMD): every wave issues iters x 16 of them (x 32768 flop).  bench.py times the launch for `roofline.mfma_stream`
 * -- the power / clock ceiling of the matrix pipes on the box the bench runs on (csrc/probe.hip).  sink: >= 1 float. */
int nbdt_probe_mfma_stream(int32_t blocks, int32_t iters, float* sink, void* stream);
/* LDS-operand MFMA streams: the dense K loop's ds_read_b128 + MFMA mix with no LDS-DMA, barriers or epilogue, for the
 * production tiling (variant 0: 8 waves x 64 pixels x 160 couts, 14 reads per 20 MFMAs) and for the one-wave-per-SIMD
 * tiling (variant 1: 4 waves x 128 pixels x 160 couts, 18 reads per 40 MFMAs, software-pipelined).  160 MFMAs per CU and
 * step either way: flops = blocks x iters x 160 x 32768.  Measurement only. */
int nbdt_probe_lds_mfma(int32_t blocks, int32_t iters, int32_t variant, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NBDT_HIP_H */
