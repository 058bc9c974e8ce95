/*
 * checkerpose_hip.h -- C ABI of libcheckerpose_hip.so (MI355X / gfx950).
 *
 * The reference (RuyiLian/CheckerPose) has NO native code and NO FFI: its hot path is the torch-op
 * sequence inside InitNet_GNN.forward / PoseNet_GNNskip.forward.  Each entry point below therefore
 * replaces a span of reference Python (cited per function, paths relative to
 * /root/reference/checkerpose) rather than an existing foreign function.  The binding a maintainer
 * adds on the reference side is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + ints, no torch / HIP types in signatures; `cp_stream_t` is a hipStream_t
 *     passed as void* (NULL = default stream).
 *   - every buffer (activations, packed weights, outputs) is caller-owned DEVICE memory; the
 *     library allocates nothing and is re-entrant and stream-ordered.  Its only process state: the thread-local
 *     cp_last_kernel note, and idempotent per-DEVICE caches (an atomic bit per device ordinal = "the large-LDS
 *     function attributes are set on this device", the device's CU count) -- calls are made on the caller's
 *     current device (hipSetDevice), several devices and several threads per process are fine.
 *   - activations are channels-last: (B, H, W, Cphys) with Cphys a multiple of cp_chan_align(dtype);
 *     padded channels are zero.  Graph features are (B, N, Cphys), i.e. the same layout with H=1.
 *   - returns CP_OK (0) or a negative code; cp_strerror() names it.
 */
#ifndef CHECKERPOSE_HIP_H
#define CHECKERPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cp_stream_t;

/* CP_F16 (IEEE half storage, f16 MFMA, fp32 accumulate; values saturate at +-65504): accepted ONLY by the keypoint-side entry
 * points that say so (cp_edgeconv_fused_t, cp_edgeconv_tiled_t, cp_mlp_pair_fused*_t, cp_mlp_query_fused_t, cp_index2feat_conv_t,
 * cp_pack_gemm_weight, cp_conv2d_igemm with CpConvDesc.dtype = CP_F16 / out_f32 = 2) -- the bf16 program runs its per-keypoint
 * (GNN) block group in f16: same bytes and MFMA rate, 3 more mantissa bits where EdgeConv's neighbour differences cancel. */
enum { CP_F32 = 0, CP_BF16 = 1, CP_F16 = 2 };
enum { CP_ACT_NONE = 0, CP_ACT_RELU = 1, CP_ACT_LEAKY = 2 };
enum { CP_LOSS_BCE = 0, CP_LOSS_L1 = 1 };   /* loss_type of losses/code_loss.py ("CE": cp_masked_ce_loss) */
enum {
  CP_OK = 0,
  CP_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  CP_ERR_HIP = -2,       /* a HIP runtime call failed (launch error, bad pointer, ...) */
  CP_ERR_ALIGN = -3,     /* pointer or stride not aligned as the kernel requires */
  CP_ERR_RANGE = -4      /* buffer too large for 32-bit buffer addressing (>= 2 GiB), or a size beyond a launch-grid dimension */
};

int cp_version(void);
const char* cp_strerror(int code);
/* profiling aid: symbol of the HIP kernel the calling thread's most recent entry point launched, spelled as
 * rocprofv3 --kernel-trace prints it (e.g. "conv_igemm_kernel<BF16Tag, 2, 4>"); "" before the first launch. */
const char* cp_last_kernel(void);
/* the same for entry points that issue SEVERAL launches (cp_edgeconv_tiled: key table + gather): cp_kernel_log_begin() clears the
 * calling thread's log, cp_kernel_log() returns every symbol launched since, joined by " + " in launch order (the log is bounded:
 * 1 KB, later symbols are dropped) -- bench.py prices such a call as the SET of its launches. */
void cp_kernel_log_begin(void);
const char* cp_kernel_log(void);

/* Deterministic training mode (process-wide switch; default off).  The reference's step (train.py:303-320) is deterministic on
 * CPU; the default training entry points here accumulate BatchNorm sums, small weight gradients and Index2Feat's scatter with
 * floating-point atomics, whose order varies from run to run.  With the switch on: cp_bn_* accumulate one block per accumulator
 * set (cp_bn_acc_doubles() grows to 64 sets; consumers add the sets in index order), cp_conv2d_wgrad_* always go through partial
 * tiles + the fixed-order reduction (a call without a workspace is refused: CP_ERR_INVALID), cp_index2feat_gather_bwd* sums each
 * patch pixel's contributions in keypoint order.  Same inputs + same launch plan => bit-identical gradients.  The switch is
 * read when an entry point is CALLED (and when a size query is answered): set it before building launch programs / graphs and
 * rebuild them after changing it.  The eval path has no atomics and ignores it. */
void cp_set_deterministic(int on);
int cp_get_deterministic(void);

/* Device-side error channel: one sticky status word per device, OR-ed into by kernels that can detect a failure of their own, read by
 * the host wherever it synchronises anyway (the drop-in models: program build, invalidate(), check_device_status()).  The call
 * synchronises the device (a plain hipMemcpy), creates the word on first use (call it once OUTSIDE a stream capture before launching
 * -- the models do) and, with clear != 0, resets a non-zero word.  Bits:
 *   CP_STATUS_CHAIN0_HANDOVER  the pipelined 64 x 64 chain (cp_hr_branch_chain*, hr_chain0p_kernel) gave up a bounded wait for a row
 *                              hand-over between its waves: that launch's output is WRONG (the bound keeps the box alive, this bit
 *                              keeps the result honest)
 *   CP_STATUS_CHAIN0_STAGING   the same kernel's staging / tail loop ran out of its bound before finishing its rows */
enum { CP_STATUS_CHAIN0_HANDOVER = 1, CP_STATUS_CHAIN0_STAGING = 2 };
int cp_device_status(uint32_t* status_out, int clear);

/* elements per 16 bytes: 4 (f32) or 8 (bf16).  Physical channel counts are multiples of this. */
int cp_chan_align(int dtype);

/* ---------------------------------------------------------------------------------------------
 * Weight packing (init / load_state_dict time, not the hot path).
 * Packs a PyTorch-layout fp32 weight into MFMA-fragment order for cp_conv2d_igemm:
 *   K index = (r, s, cin) with cin padded to cin_phys; blocks of 1 KiB = one (16-channel tile,
 *   K-chunk) wave fragment, ordered [tile][chunk][lane][16 B].
 * transposed = 0 : w is (Cout, Cin, R, S)      (nn.Conv2d / nn.Linear with R=S=1)
 * transposed = 1 : w is (Cin, Cout, 3, 3) of ConvTranspose2d(k3,s2,p1,op1) (pipeline.py:187-197) and
 *                  `phase` = 2*a+b selects the sub-pixel phase (output row parity a, column parity b);
 *                  the packed kernel then has R=1+a, S=1+b taps.
 * row_map (optional, length cout_rows): packed output row n takes source row row_map[n] (or zeros if
 *   row_map[n] < 0); NULL = identity.  Used to interleave zero rows (init MLP, init.py:107).
 * ------------------------------------------------------------------------------------------- */
size_t cp_packed_weight_bytes(int dtype, int cout_rows, int cin_phys, int R, int S);
int cp_pack_conv_weight(cp_stream_t stream, int dtype, const float* w, int Cout, int Cin, int R, int S,
                        int cin_phys, int transposed, int phase, const int32_t* row_map, int cout_rows,
                        void* packed);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA (fp32: v_mfma_f32_16x16x4_f32, bf16: v_mfma_f32_16x16x32_bf16),
 * fused per-channel affine (folded BatchNorm or bias), optional residual add, activation.
 * Replaces every nn.Conv2d(+BatchNorm2d)(+ReLU/LeakyReLU) and nn.Linear on the path:
 *   backbone convs (timm hrnet/resnet via backbone.py:48), init.py:85-95 (conv1x1), init.py:58-62 +
 *   pipeline.py:49-53 (EdgeConv 1x1 conv, in its factored per-node form), init.py:107 (mlp),
 *   pipeline.py:183-211 (decoder), pipeline.py:146-147 (patch_generator), pipeline.py:61-69,168-180
 *   (MLPs), pipeline.py:349 (seg_block).
 *
 *   out[o_base + b*o_sb + oy*o_sy + ox*o_sx + c*o_sc] =
 *       act( conv(in)[b,oy,ox,c] * scale[c] + shift[c] + residual[same index] )
 * ------------------------------------------------------------------------------------------- */
typedef struct CpConvDesc {
  int32_t dtype;          /* CP_F32 | CP_BF16: type of in / packed weights / residual / out */
  int32_t out_f32;        /* 1: out (and residual) are fp32 regardless of dtype (final logits, seg); 2 (cp_conv2d_igemm, cp_conv2x2_halo,
                             dtype CP_BF16, no residual): out rows are IEEE half (CP_F16: the producer of a keypoint-side tensor) */
  int32_t B, H, W;        /* input spatial size */
  int32_t Cin;            /* channels contracted (physical, multiple of cp_chan_align) */
  int32_t in_cstride;     /* elements between consecutive input pixels (>= in_coff + Cin) */
  int32_t in_coff;        /* first channel of the input slice */
  int32_t R, S, stride, pad;
  int32_t Ho, Wo;         /* output spatial size (iy = oy*stride - pad + r) */
  int32_t Cout;           /* channels stored (physical) ; weights were packed with cout_rows >= Cout */
  int32_t act;            /* CP_ACT_* */
  float slope;            /* LeakyReLU negative slope */
  int32_t ksplit;         /* cp_conv2d_igemm: -1 = never use the split-K variant (results then do not depend on the batch
                             size, bit for bit); anything else = the library decides by shape (cp_conv2d_igemm_splitk).
                             Sits in what was alignment padding: the struct's size and offsets are unchanged. */
  int64_t o_base, o_sb, o_sy, o_sx, o_sc;   /* output (and residual) element strides */
} CpConvDesc;

int cp_conv2d_igemm(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w,
                    const float* scale, const float* shift, const void* residual, void* out);
/* Small-batch routing query: 0, or the number of waves cp_conv2d_igemm would split this conv's K walk over (bf16, long K,
 * a grid that would leave most CUs idle: the split-K variant of the kernel).  M = B*Ho*Wo output pixels, K = R*S*Cin with
 * Cin the PHYSICAL input channels, Cout the physical output channels.  A host that has a specialised large-batch kernel
 * for the layer (halo / row-GEMM) asks this first and, if non-zero, packs the generic weight image instead. */
int cp_conv2d_igemm_splitk(int dtype, long long M, int K, int Cout);

/* ---------------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 specialisation with an LDS-staged input halo tile (decoder convs pipeline.py:183-211,
 * HRNet/ResNet body convs): same arithmetic and descriptor as cp_conv2d_igemm (requires R=S=3, stride=1, pad=1,
 * o_sc=1, out_f32=0) but its own packed-weight image ([32-ch group][chunk][tap][tile][lane][16 B], rows permuted
 * for 16-byte epilogue stores).  scale/shift must be readable 8 floats at a time (pad to a multiple of 8).
 * ------------------------------------------------------------------------------------------- */
size_t cp_packed_halo_weight_bytes(int dtype, int Cout, int cin_phys);
int cp_pack_conv3x3_halo_weight(cp_stream_t stream, int dtype, const float* w, int Cout, int Cin, int cin_phys,
                                void* packed);
int cp_conv3x3_halo(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w,
                    const float* scale, const float* shift, const void* residual, void* out);
/* k = 2 / stride 1 / pad 1 conv with <= 80 output channels off the same LDS-staged halo tile (Index2Feat_module.patch_generator,
 * pipeline.py:144-145,156, where it runs over the whole map: N = 4096 keypoints, the low-resolution stages at N = 512): descriptor as
 * cp_conv2d_igemm with R = S = 2, stride 1, pad 1, Ho = H + 1, Wo = W + 1, o_sc = 1; weights by cp_pack_conv2x2_halo_weight from the
 * fp32 (Cout, Cin, 2, 2) tensor; scale / shift / residual / activation as cp_conv3x3_halo. */
int cp_conv2x2_halo_supported(int dtype, int H, int W, int Cout_phys);
size_t cp_packed_conv2x2_halo_weight_bytes(int dtype, int Cout, int Cin_phys);
int cp_pack_conv2x2_halo_weight(cp_stream_t stream, int dtype, const float* w, int Cout, int Cin, int cin_phys, void* packed);
int cp_conv2x2_halo(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w, const float* scale,
                    const float* shift, const void* residual, void* out);

/* conv3x3( UpsamplingBilinear2d(scale_factor=2)(in) ) without the upsampled tensor: the decoder's `up_net[1..2]` upsample + first
 * conv (pipeline.py:199-200, get_gdrn_upsample_module).  Descriptor as cp_conv3x3_halo, except that d->H, d->W (= Ho, Wo, both
 * even) are the UPSAMPLED size and `in` is the (B, H/2, W/2, in_cstride) source; Cout a multiple of 256 (the wide kernel), no
 * residual.  Each halo pixel is interpolated (align_corners=True, the arithmetic of cp_upsample2x_bilinear_ac bit for bit) while
 * the tile is staged.  Weights: cp_pack_conv3x3_halo_weight. */
int cp_conv3x3_halo_up2x_supported(int dtype, int Cout);
int cp_conv3x3_halo_up2x(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w,
                         const float* scale, const float* shift, void* out);

/* conv3x3/s1/p1 + folded BN + act (Cout == 256) WITH the 1x1 head that reads its output fused into the epilogue: the decoder's
 * last conv + `seg_block` (pipeline.py:349,383: Conv2d(256 -> S) + bias on the last feature map).  `out` is written as by
 * cp_conv3x3_halo; seg_out (B, S, H, W) fp32 NCHW = seg_b[s] + sum_c seg_w[s][c] * out[b, y, x, c] (the stored, i.e.
 * dtype-rounded, activations; seg_w = [S][256] fp32, pre-rounded to `dtype` by the caller).  S <= 2. */
int cp_conv3x3_halo_seg_supported(int dtype, int Cout, int S);
int cp_conv3x3_halo_seg(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w, const float* scale,
                        const float* shift, void* out, const float* seg_w, const float* seg_b, int S, float* seg_out);

/* 3x3 / stride 2 / pad 1 convolution with a wide input and at most 48 output channels (bf16): HRNet `transition1[1]`
 * (256 -> 36 at 64 x 64 -> 32 x 32; timm HighResolutionNet.transition1 inside backbone.py:48-49).  Descriptor as
 * cp_conv2d_igemm with R = S = 3, stride 2, pad 1, Ho = H / 2, Wo = W / 2; H a multiple of 8, W in {32, 64}, Cin a multiple of
 * 32, d->Cout = physical output channels (multiple of 8, <= 48), scale / shift padded to a multiple of 16 floats.  A
 * workgroup stages 8 input rows of one 32-channel chunk in LDS (every input byte is fetched 9/8 times instead of 2.4). */
int cp_conv3x3_s2_small_supported(int H, int W, int cin_phys, int out_cphys);
size_t cp_conv3x3_s2_small_weight_bytes(int cin_phys, int out_cphys);
int cp_pack_conv3x3_s2_small_weight(cp_stream_t stream, const float* w, int Cout, int Cin, int cin_phys, int out_cphys, void* packed);
int cp_conv3x3_s2_small(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w, const float* scale,
                        const float* shift, void* out);

/* Fused timm BasicBlock of the HRNet branches (C -> C channels, C <= 32 and one 64-byte chunk, stride 1):
 *   out = relu( conv3x3(relu(conv3x3(x)*s1+t1))*s2+t2 + x )     -- intermediate and residual never leave LDS.
 * packed_w1: cp_pack_conv3x3_rows_weight (unpermuted rows); packed_w2: cp_pack_conv3x3_halo_weight.
 * Descriptor as cp_conv3x3_halo with Cin == Cout; `out` must not alias `in`. */
int cp_pack_conv3x3_rows_weight(cp_stream_t stream, int dtype, const float* w, int Cout, int Cin, int cin_phys,
                                void* packed);
int cp_basicblock_fused(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w1,
                        const float* scale1, const float* shift1, const void* packed_w2, const float* scale2,
                        const float* shift2, void* out);

/* timm resnet.Bottleneck of HRNet layer1 (inside timm.create_model, backbone.py:35) in ONE launch:
 *   out = relu( bn3(conv1x1( relu(bn2(conv3x3( relu(bn1(conv1x1(x))) ))) )) + shortcut(x) ),  Cin -> 64 -> 64 -> 256
 *   blocks 1..3: Cin = 256, shortcut = identity (packed_wd = scaled = shiftd = NULL);
 *   block 0    : Cin = 64,  shortcut = bn_d(conv1x1_d(x)) (`downsample`), packed_wd (256,64,1,1) + its folded BN.
 * bf16 storage only (the x halo tile, both intermediates and the output tile live in <= 140 KB of LDS).  d: dtype
 * CP_BF16, Cin as above, Cout = 256, stride 1, H/W/B, input slice and output strides as for cp_conv2d_igemm;
 * in != out.  All weights in the generic image of cp_pack_conv_weight: w1 (64,Cin,1,1) cin_phys Cin; w2 (64,64,3,3)
 * cin_phys 64; w3 / wd (256,64,1,1) cin_phys 64.  scale/shift: folded BatchNorm (64, 64, 256, 256 floats, 16-byte
 * aligned). */
int cp_bottleneck_fused(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w1,
                        const float* scale1, const float* shift1, const void* packed_w2, const float* scale2,
                        const float* shift2, const void* packed_w3, const float* scale3, const float* shift3,
                        const void* packed_wd, const float* scaled, const float* shiftd, void* out);

/* ---------------------------------------------------------------------------------------------
 * 1x1 conv / Linear specialisation with LDS-staged rows (EdgeConv node GEMMs, 256-wide MLPs pipeline.py:61-69,
 * 168-180, conv1x1 init.py:85-95, incre conv3): same arithmetic and descriptor as cp_conv2d_igemm (requires
 * R=S=1, stride=1, pad=0, o_sc=1, out_f32=0), own packed image ([32-ch group][chunk][tile][lane][16 B]).
 * ------------------------------------------------------------------------------------------- */
size_t cp_packed_gemm_weight_bytes(int dtype, int Cout, int cin_phys);
int cp_pack_gemm_weight(cp_stream_t stream, int dtype, const float* w, int Cout, int Cin, int cin_phys, void* packed);
int cp_gemm_rows(cp_stream_t stream, const CpConvDesc* d, const void* in, const void* packed_w,
                 const float* scale, const float* shift, const void* residual, void* out);

/* MLP_QueryNet.forward (pipeline.py:168-180: Linear(256 -> 256) + LeakyReLU, Linear(256 -> 64) + LeakyReLU, Linear(64 -> 2); the
 * `pts` argument is unused there) as ONE launch over the B * N keypoint rows, bf16: rows read once, both hidden layers stay on chip
 * (LDS / registers), only the two logits per row leave.  in (B, N, in_cstride) bf16 channels [in_coff, in_coff + 256);
 * packed_w1 / packed_w2: cp_pack_gemm_weight images of the (256, 256) and (64, 256) weights, scale / shift fp32 per output channel
 * (nn.Linear: scale 1, shift = bias); w3 fp32 (2, 64) row-major as nn.Linear stores it, b3 fp32 (2).
 * out fp32: logit c of row (b, n) at out[o_base + b * o_sb + n * o_sn + c * o_sc] (the (B, 13, N) logit block: pipeline.py:375-378). */
int cp_mlp_query_fused_supported(int C0, int C1, int C2, int C3);
int cp_mlp_query_fused(cp_stream_t stream, const void* in, int in_cstride, int in_coff, int B, int N,
                       const void* packed_w1, const float* scale1, const float* shift1, float slope1,
                       const void* packed_w2, const float* scale2, const float* shift2, float slope2,
                       const float* w3, const float* b3, float* out, long long o_base, long long o_sb, long long o_sn, long long o_sc);
/* the same with the rows, both packed weight images (cp_pack_gemm_weight(dtype, ...)) and the on-chip hidden rows in `dtype` = CP_BF16 or CP_F16 */
int cp_mlp_query_fused_t(cp_stream_t stream, int dtype, const void* in, int in_cstride, int in_coff, int B, int N,
                         const void* packed_w1, const float* scale1, const float* shift1, float slope1,
                         const void* packed_w2, const float* scale2, const float* shift2, float slope2,
                         const float* w3, const float* b3, float* out, long long o_base, long long o_sb, long long o_sn, long long o_sc);
/* the same with `nout` logits per row: 2 (the above) or 1 + 2r, r = 4..6 -- the woProg ablation's single head
 * (pipeline_lm.py:475-517); cp_mlp_query_fused_supported(256, 256, 64, nout) says which.  w3 fp32 (nout, 64), b3 fp32 (nout).
 * With x_id64 / y_id64 (both or neither; nout = 1 + 2r only) the same launch decodes the x / y codes -- logit rows 1..r and
 * r+1..2r, MSB first, bit = [z > CP_SIGMOID_HALF_Z0] exactly as cp_bits_decode -- into ids (B, N) int64 (from_code_prob_to_id,
 * pipeline.py:84-92), and into x_id32 / y_id32 (B, N) int32 where given. */
int cp_mlp_query_fused_n(cp_stream_t stream, int dtype, const void* in, int in_cstride, int in_coff, int B, int N,
                         const void* packed_w1, const float* scale1, const float* shift1, float slope1,
                         const void* packed_w2, const float* scale2, const float* shift2, float slope2,
                         const float* w3, const float* b3, int nout, float* out, long long o_base, long long o_sb, long long o_sn,
                         long long o_sc, int64_t* x_id64, int64_t* y_id64, int32_t* x_id32, int32_t* y_id32);

/* Refine_moduleGNN.pre_graph_module (pipeline.py:237-240, applied at :283-286: Linear(Cin -> 256) + LeakyReLU, Linear(256 -> 256) +
 * LeakyReLU over the concatenated [local | previous graph] feature rows) as ONE launch, bf16: the hidden rows stay in LDS.
 * in (B, N, in_cstride) channels [in_coff, in_coff + Cin), Cin a multiple of 32, <= 512; packed_w1 / packed_w2: cp_pack_gemm_weight
 * images of the (256, Cin) and (256, 256) weights; bias fp32 (256) each; out (B, N, out_cstride) channels [out_coff, out_coff + 256). */
int cp_mlp_pair_fused_supported(int Cin, int C1, int C2);
int cp_mlp_pair_fused(cp_stream_t stream, const void* in, int in_cstride, int in_coff, int Cin, int B, int N,
                      const void* packed_w1, const float* bias1, float slope1, const void* packed_w2, const float* bias2, float slope2,
                      void* out, int out_cstride, int out_coff);
/* ... in `dtype` = CP_BF16 or CP_F16 (input rows, weights, hidden rows, output rows) */
int cp_mlp_pair_fused_t(cp_stream_t stream, int dtype, const void* in, int in_cstride, int in_coff, int Cin, int B, int N,
                        const void* packed_w1, const float* bias1, float slope1, const void* packed_w2, const float* bias2,
                        float slope2, void* out, int out_cstride, int out_coff);

/* The same with Index2Feat_module's gather (pipeline.py:156-163: four 64-channel taps of patch_generator's output map at
 * (2v, 2u), (2v + k, 2u), (2v, 2u + k), (2v + k, 2u + k), times the {0, 1} RoI bit, :280) done by the kernel's DMA loader: the
 * (B, N, 256) local-feature tensor is never written or read back.  Row (b, n) = [tap 0 | tap 1 | tap 2 | tap 3 | gin row], i.e. the
 * weight packed_w1 is the (256, 256 + Cg) one of cp_mlp_pair_fused.  patches (B, Hp, Wp, p_cstride) bf16, channels
 * [p_coff, p_coff + 64); x_id / y_id int32 (B, N), mask fp32 (B, N) as cp_bits_decode leaves them; zeros: >= 128 zero bytes (the
 * source of rows whose RoI bit is 0); gin (B, N, gin_cstride) channels [gin_coff, gin_coff + Cg), Cg in {64, 128, 192, 256}. */
typedef struct {
  const void* patches;
  const int32_t* x_id;
  const int32_t* y_id;
  const float* mask;
  const void* zeros;
  int32_t p_cstride, p_coff, Hp, Wp, k;
} CpI2fGather;
int cp_mlp_pair_fused_gather_supported(int Cg, int E_ch, int k);
int cp_mlp_pair_fused_gather(cp_stream_t stream, const CpI2fGather* g, const void* gin, int gin_cstride, int gin_coff, int Cg, int B, int N,
                             const void* packed_w1, const float* bias1, float slope1, const void* packed_w2, const float* bias2,
                             float slope2, void* out, int out_cstride, int out_coff);
/* ... in `dtype` = CP_BF16 or CP_F16 (patch map, graph rows, weights, hidden rows, output rows: ONE type) */
int cp_mlp_pair_fused_gather_t(cp_stream_t stream, int dtype, const CpI2fGather* g, const void* gin, int gin_cstride, int gin_coff, int Cg,
                               int B, int N, const void* packed_w1, const float* bias1, float slope1, const void* packed_w2,
                               const float* bias2, float slope2, void* out, int out_cstride, int out_coff);

/* nn.UpsamplingBilinear2d(scale_factor=2) == interpolate(align_corners=True), pipeline.py:199.
 * Reads channels [in_coff, in_coff+C) of (B,H,W,in_cstride), writes [out_coff, ..) of (B,2H,2W,out_cstride).
 * H == 1 / W == 1 are legal (scale 0: both outputs of the axis copy the one input).  The source coordinate is ATen's float32
 * scale * dst on an axis of up to 128 inputs and the exact quotient on a longer one (the float32 product is off by about
 * n * 2^-23 of a pixel); cp_conv3x3_halo_up2x and the backward follow the same rule.  CP_ERR_INVALID: a channel slice outside
 * [0, cstride), negative offsets included. */
int cp_upsample2x_bilinear_ac(cp_stream_t stream, int dtype, const void* in, void* out, int B, int H, int W,
                              int C, int in_cstride, int in_coff, int out_cstride, int out_coff);

/* HRNet fuse layer sum (timm HighResolutionModule.forward): out = relu?( sum_t nearest_up(src_t, 2^shift_t) ),
 * sources (B, H>>shift_t, W>>shift_t, C) contiguous, nsrc <= 4; written to channels [out_coff, out_coff + C) of the
 * (B, H, W, out_cstride) tensor `out` (out_cstride = C, out_coff = 0: a plain tensor). */
int cp_fuse_sum_act(cp_stream_t stream, int dtype, int nsrc, const void* const* srcs, const int32_t* shifts,
                    void* out, int B, int H, int W, int C, int relu, int out_cstride, int out_coff);

/* max_pool2d(3, 2, 1) for the resnet34 stem (timm resnet). (B,H,W,C) -> (B,H/2,W/2,C) */
int cp_maxpool3x3s2(cp_stream_t stream, int dtype, const void* in, void* out, int B, int H, int W, int C);

/* ---------------------------------------------------------------------------------------------
 * EdgeConv aggregation, factored form of StaticGraph_module.forward (init.py:64-68 == pipeline.py:55-59,
 * get_graph_feature init.py:36-49).  pq is the per-node GEMM output (B, N, 2*C): [P' | Q'] with the
 * BatchNorm scale folded in (P' = s*W1 x, Q' = s*(W2-W1) x + t), so
 *   out[b,i,c] = leaky( max_k P'[b, idx[g,i,k], c] + Q'[b,i,c] ),   g = graph_ids ? graph_ids[b] : 0
 * idx is (G, N, K) int32 (LM: per-object tables, pipeline_lm.py:57).  Writes channels
 * [out_coff, out_coff+C) of (B, N, out_cstride).
 * ------------------------------------------------------------------------------------------- */
int cp_edgeconv_gather_max(cp_stream_t stream, int dtype, const void* pq, const int32_t* idx,
                           const int32_t* graph_ids, void* out, int B, int N, int K, int C, int G,
                           int out_cstride, int out_coff, float slope);

/* Index2Feat_module.forward gather (pipeline.py:156-163) fused with the RoI mask multiply (pipeline.py:280):
 * patches (B, Hp, Wp, E); for keypoint (b,i) taps (2y,2x), (2y+k,2x), (2y,2x+k), (2y+k,2x+k) ->
 * out[b,i, out_coff + t*E + e] = patches[b,ty,tx,e] * mask[b,i].  ids int32 (B,N), mask fp32 (B,N). */
int cp_index2feat_gather(cp_stream_t stream, int dtype, const void* patches, const int32_t* x_id,
                         const int32_t* y_id, const float* mask, void* out, int B, int N, int Hp, int Wp,
                         int E, int k, int out_cstride, int out_coff);

/* HRNet stem in one launch (bf16): NCHW fp32 image (B, 3, Hin, Win) -> conv1 3x3/s2 (3 -> 64) + BN + ReLU -> conv2 3x3/s2
 * (64 -> 64) + BN + ReLU -> (B, Hin/4, Win/4, 64) bf16 channels-last (timm hrnet conv1/bn1/conv2/bn2 behind reference
 * backbone.py:48-49); the 2 MB-per-crop intermediate never leaves LDS.  Hin % 32 == 0, Win % 64 == 0.  Weights: fp32
 * (64, 3, 3, 3) and (64, 64, 3, 3) packed by cp_pack_hr_stem_weights into buffers of cp_hr_stem_weight_bytes(0 | 1) bytes;
 * scale / shift = folded BatchNorm, 64 floats each. */
size_t cp_hr_stem_weight_bytes(int which);
int cp_pack_hr_stem_weights(cp_stream_t stream, const float* w1, const float* w2, void* packed1, void* packed2);
int cp_hr_stem(cp_stream_t stream, const float* img_nchw, int B, int Hin, int Win, const void* packed1, const float* scale1,
               const float* shift1, const void* packed2, const float* scale2, const float* shift2, void* out);

/* ---------------------------------------------------------------------------------------------
 * One launch per HRNet branch chain (bf16): the four BasicBlocks of `HighResolutionModule.branches[j]` (inside
 * timm.create_model("hrnet_w18", features_only=True), reference backbone.py:48-49; restated oracle/checkerpose_oracle.py
 * _hr_module) preceded by the previous module's fuse sum, with the crop's whole branch map resident in LDS.
 *   x   = [relu]( sum_k upsample_nearest(src_k, 2^shift_k) )        srcs (B, H>>shift, W>>shift, Cphys) bf16, Cphys = ceil8(C)
 *   for blk in 0..3:  x = relu( bn2(conv3x3(relu(bn1(conv3x3(x))))) + x )
 *   out = x                                                           (B, H, W, Cphys) bf16, pad channels exactly zero
 * Supported (C, H, W): (18, 64, 64), (36, 32, 32), (72, 16, 16), (144, 8, 8) -- the four HRNet-W18 branches of a 256 x 256
 * crop (cp_hr_chain_supported).  The 64 x 64 branch keeps its BasicBlock residuals in `out` between blocks (its map alone fills
 * the LDS), the others keep them on chip.  Weights: cp_pack_hr_chain_weight() packs conv `conv_index` (0..7 = block.conv1, block.conv2, ...)
 * of fp32 (C, C, 3, 3) weights TIMES the folded-BN `scale` of their output channel (fp32 [C]; NULL = 1) into the caller-owned
 * blob of cp_hr_chain_weight_bytes() bytes; `affine` = fp32 [8][2][cp_hr_chain_affine_floats()] per conv, zero beyond C: row 1
 * is the folded-BN shift the accumulators start from, row 0 is NOT read (the scale lives in the weights: a block's epilogue
 * is residual + ReLU + rounding only).  out must not alias a source. */
int cp_hr_chain_supported(int C, int H, int W);
size_t cp_hr_chain_weight_bytes(int C, int H, int W);
int cp_hr_chain_affine_floats(int C, int H, int W);
int cp_pack_hr_chain_weight(cp_stream_t stream, const float* w, const float* scale, int C, int H, int W, int conv_index, void* blob);
int cp_hr_branch_chain(cp_stream_t stream, int B, int C, int H, int W, int nsrc, const void* const* srcs,
                       const int32_t* shifts, int relu_in, const void* packed_w, const float* affine, void* out);

/* cp_hr_branch_chain of the 64 x 64 x 18 branch WITH the stride-2 fuse-layer convs that read its output (kind 1 of cp_hr_fuse_out
 * below: fuse_layers[i][0][0], i = 1..3, 3x3 / stride 2 / pad 1 + folded BN (+ ReLU where the down-sampling chain goes on)) computed
 * off the finished map while it is still in LDS: the separate launch behind the module's longest chain and its re-read of the map
 * disappear.  Up to 3 convs whose padded channel counts (out_cphys, multiples of 8) add up to <= cp_hr_chain_tail_channels() (96:
 * HRNet-W18 has 40 + 24 + 24); conv i owns the 16-byte channel pieces [first_piece_i, first_piece_i + out_cphys_i / 8) with
 * first_piece_0 = 0 and first_piece_{i+1} = first_piece_i + out_cphys_i / 8.
 *   packed_w: one ZERO-FILLED blob of cp_hr_chain_tail_weight_bytes() bytes into which cp_pack_hr_chain_tail_weight() has written every
 *             conv (fp32 (Cout, 18, 3, 3) weights TIMES the folded-BN scale of their output channel);
 *   shift:    fp32 [96], the folded-BN shift at combined channel 8 * first_piece_i + c, zero elsewhere;
 *   out[i]:   (B, 32, 32, out_cphys[i]) bf16, channels [Cout, out_cphys) exactly zero.
 * Same arithmetic as the chain's own convs (bf16 operands with the scale folded in, fp32 accumulate starting from the shift). */
typedef struct CpChainTail {
  const void* packed_w;
  const float* shift;
  void* out[3];
  int32_t nconv;
  int32_t Cout[3], out_cphys[3], relu[3];
} CpChainTail;
int cp_hr_chain_tail_supported(int C, int H, int W);
size_t cp_hr_chain_tail_weight_bytes(void);
int cp_hr_chain_tail_channels(void);
int cp_pack_hr_chain_tail_weight(cp_stream_t stream, const float* w, const float* scale, int Cout, int first_piece, int out_cphys, void* blob);
int cp_hr_branch_chain_tail(cp_stream_t stream, int B, int C, int H, int W, int nsrc, const void* const* srcs,
                            const int32_t* shifts, int relu_in, const void* packed_w, const float* affine, void* out,
                            const CpChainTail* tail);

/* The same for the 36 / 72 / 144-channel chains (round 5): ANY first-level fuse-layer conv that reads the branch -- kind 0: the 1x1
 * conv + BN towards a higher-resolution branch (output at the branch's resolution), kind 1: the first 3x3 / stride-2 conv + BN
 * (+ ReLU when the chain goes on) towards a lower-resolution one (output at half resolution) -- runs in the chain launch's tail off
 * the map in LDS: the grouped cp_hr_fuse_out launch behind the chain and its re-read of the map go away.  Up to 3 convs per launch;
 * weights packed by cp_pack_hr_chain_tailconv_weight (folded-BN scale inside), shift: fp32 [16 ceil(Cout / 16)] (zero beyond Cout);
 * out (B, H >> kind, W >> kind, out_cphys) bf16, out_cphys a multiple of 8 in [Cout, 16 ceil(Cout / 16)].  Supported (kind, Cout)
 * pairs are HRNet-W18's: C = 36: 1x1 -> 18, s2 -> 72 / 36; C = 72: 1x1 -> 18 / 36, s2 -> 144; C = 144: 1x1 -> 18 / 36 / 72. */
typedef struct {
  const void* packed_w;
  const float* shift;
  void* out;
  int32_t kind, Cout, out_cphys, relu;
} CpChainTailConv;
int cp_hr_chain_tailconv_supported(int C, int H, int W, int kind, int Cout);
size_t cp_hr_chain_tailconv_weight_bytes(int C, int H, int W, int kind, int Cout);
int cp_pack_hr_chain_tailconv_weight(cp_stream_t stream, const float* w, const float* scale, int C, int H, int W, int kind, int Cout,
                                     void* packed);
int cp_hr_branch_chain_tails(cp_stream_t stream, int B, int C, int H, int W, int nsrc, const void* const* srcs, const int32_t* shifts,
                             int relu_in, const void* packed_w, const float* affine, void* out, int ntail, const CpChainTailConv* convs);

/* The first-level fuse-layer convs of a timm HighResolutionModule that read ONE branch's output `src` (B, H, W, cin_phys) bf16
 * (timm HighResolutionModule.fuse_layers inside backbone.py:35): up to 4 convs per launch, each
 *   kind 0: 1x1 conv + folded BN at the source resolution (the term towards a higher-resolution branch, before its nearest
 *           upsample), or
 *   kind 1: 3x3 / stride 2 / pad 1 conv + folded BN (+ ReLU when `relu`: a chain that goes on) at half the resolution,
 * out_i = act(conv_i(src) * scale + shift) as (B, Ho, Wo, out_cphys) bf16, channels [Cout, out_cphys) exactly zero.  A
 * workgroup stages a band of src in LDS once and runs every conv off it.  packed_w: cp_pack_hr_fuse_out_weight of the fp32
 * (Cout, Cin, k, k) weight; affine: fp32 [2][cp_hr_fuse_out_affine_floats(out_cphys)] = scale then shift, zero beyond Cout. */
typedef struct CpFuseConv {
  const void* packed_w;
  const float* affine;
  void* out;
  int32_t kind, Cout, out_cphys, relu;
} CpFuseConv;
int cp_hr_fuse_out_supported(int H, int W, int cin_phys);
size_t cp_hr_fuse_out_weight_bytes(int cin_phys, int out_cphys, int kind);
int cp_hr_fuse_out_affine_floats(int out_cphys);   /* 0: that many (padded) output channels are not supported (> 160) */
int cp_pack_hr_fuse_out_weight(cp_stream_t stream, const float* w, int Cout, int Cin, int cin_phys, int out_cphys, int kind,
                               void* packed);
int cp_hr_fuse_out(cp_stream_t stream, const void* src, int B, int H, int W, int cin_phys, int nconv, const CpFuseConv* convs);

/* EdgeConv layer in ONE launch for N = 512 keypoints (bf16): per-node GEMM [P' | Q'] = x . wpq^T on MFMA, P' table of one
 * 64-channel slice in LDS, neighbour gather-max out of LDS, + Q', LeakyReLU (StaticGraph_module, init.py:54-68 ==
 * pipeline.py:45-59; per-sample graphs `knn_idx[obj_ids-1]` of pipeline_lm.py:55-57 through graph_ids).
 *   x (B, 512, in_cstride) channels [in_coff, in_coff + Cin);  wpq fp32 (2 Cout, Cin) = [W1 ; W2 - W1], packed by
 *   cp_pack_edgeconv_fused_weight;  scale / shift fp32 [2 Cout] = [s | s], [0 | t] (folded BatchNorm);  idx int32 (G, 512, K);
 *   out (B, 512, out_cstride) channels [out_coff, out_coff + Cout) = leaky(max_k (s W1 x)_{idx[k]} + s (W2 - W1) x + t).
 * Supported: N = 512, K <= 20 and a multiple of 4, Cin in {64, 256}, Cout in {64, 128, 192, 256} (cp_edgeconv_fused_supported);
 * other shapes (N = 4096) use cp_conv2d_igemm / cp_gemm_rows + cp_edgeconv_gather_max. */
int cp_edgeconv_fused_supported(int N, int K, int Cin, int Cout);
size_t cp_edgeconv_fused_weight_bytes(int Cin, int Cout);
int cp_pack_edgeconv_fused_weight(cp_stream_t stream, const float* wpq, int Cin, int Cout, void* packed);
int cp_edgeconv_fused(cp_stream_t stream, const void* x, int in_cstride, int in_coff, const void* packed_w,
                      const float* scale, const float* shift, const int32_t* idx, const int32_t* graph_ids, void* out,
                      int out_cstride, int out_coff, int B, int N, int K, int Cin, int Cout, int G, float slope);
/* ... in `dtype` = CP_BF16 or CP_F16 (x rows, packed weights, output rows; the gather keys are IEEE halves either way) */
int cp_pack_edgeconv_fused_weight_t(cp_stream_t stream, int dtype, const float* wpq, int Cin, int Cout, void* packed);
int cp_edgeconv_fused_t(cp_stream_t stream, int dtype, const void* x, int in_cstride, int in_coff, const void* packed_w,
                        const float* scale, const float* shift, const int32_t* idx, const int32_t* graph_ids, void* out,
                        int out_cstride, int out_coff, int B, int N, int K, int Cin, int Cout, int G, float slope);

/* EdgeConv layer for LARGE graphs (N = 1024 .. 32768 keypoints in patches of 512, bf16; BASELINE config #5: npt = 4096), the
 * LDS-staged gather of cp_edgeconv_fused, tiled (edgeconv_tiled.hip; same reference lines as above).  The caller works in an
 * INTERNAL keypoint numbering in which every patch of 512 consecutive rows is spatially compact (checkerpose_amd/graph_sched.py:
 * tile_schedule) and passes, per graph g and patch t:
 *   halo int32 (G, N/512, HPAD): internal row ids of the patch's out-of-patch neighbour rows (padded with any valid row);
 *   nbr  int16 (G, N/512, 512, K): every own row's K neighbours as table SLOTS (own row j -> j, halo entry h -> 512 + h).
 * Two launches: the key table P' = s W1 x of every row (written to `key_table`, cp_edgeconv_tiled_table_bytes, plane-major
 * [crop][Cout / 8][N][16 B] IEEE half-precision keys, clamped to +-65504), then per (crop, patch) the table slice in LDS by LDS-DMA, gather-max,
 * Q' on MFMA, LeakyReLU.  x / out / scale / shift as cp_edgeconv_fused; packed_w_fused = cp_pack_edgeconv_fused_weight's image,
 * packed_w_q = cp_pack_edgeconv_tiled_weight's (Q halves in 32-channel slices).
 * Supported (cp_edgeconv_tiled_supported): N a multiple of 512 above 512, K <= 20 and a multiple of 4, Cin in {64, 256},
 * Cout in {64 .. 256 step 64}, HPAD a multiple of 64 with the table in 160 KB of LDS (HPAD <= 1024 at Cin = 256). */
int cp_edgeconv_tiled_supported(int N, int K, int Cin, int Cout, int HPAD);
size_t cp_edgeconv_tiled_weight_bytes(int Cin, int Cout);
size_t cp_edgeconv_tiled_table_bytes(int B, int N, int Cout);
int cp_pack_edgeconv_tiled_weight(cp_stream_t stream, const float* wpq, int Cin, int Cout, void* packed);
int cp_edgeconv_tiled(cp_stream_t stream, const void* x, int in_cstride, int in_coff, const void* packed_w_fused,
                      const void* packed_w_q, const float* scale, const float* shift, const int32_t* halo,
                      const int16_t* nbr, const int32_t* graph_ids, void* key_table, void* out, int out_cstride, int out_coff,
                      int B, int N, int K, int Cin, int Cout, int G, int HPAD, float slope);
/* ... in `dtype` = CP_BF16 or CP_F16 (x rows, both packed weight images, output rows; the key table holds IEEE halves either way) */
int cp_pack_edgeconv_tiled_weight_t(cp_stream_t stream, int dtype, const float* wpq, int Cin, int Cout, void* packed);
int cp_edgeconv_tiled_t(cp_stream_t stream, int dtype, const void* x, int in_cstride, int in_coff, const void* packed_w_fused,
                        const void* packed_w_q, const float* scale, const float* shift, const int32_t* halo, const int16_t* nbr,
                        const int32_t* graph_ids, void* key_table, void* out, int out_cstride, int out_coff, int B, int N, int K,
                        int Cin, int Cout, int G, int HPAD, float slope);
/* The renumbering at the launch program's boundary (perm int32 (G, N): internal row i = original keypoint perm[g][i];
 * graph_ids (B) or NULL).  Rows of `row_bytes` (a multiple of 16): out[b][i] = in[b][perm[g_b][i]].  Columns of (B, R, N)
 * arrays of 4- / 8-byte elements (logit block, ids): scatter = 1: out[b][r][perm[g_b][i]] = in[b][r][i] (internal -> original),
 * scatter = 0: out[b][r][i] = in[b][r][perm[g_b][i]].  Not in place (in == out: CP_ERR_INVALID). */
int cp_permute_rows(cp_stream_t stream, const void* in, void* out, const int32_t* perm, const int32_t* graph_ids, int B, int N,
                    int row_bytes);
int cp_permute_cols(cp_stream_t stream, const void* in, void* out, const int32_t* perm, const int32_t* graph_ids, int B, int R,
                    int N, int elem_bytes, int scatter);

/* Index2Feat_module.forward + RoI mask in one launch (bf16): the patch_generator conv (Conv2d(256 -> 64, k = 2, pad = 1),
 * pipeline.py:146-147) evaluated ONLY at the 4 gathered taps of every keypoint (pipeline.py:156-163), times mask (pipeline.py:280):
 *   out[b, n, 64 t + c] = mask[b, n] * (bias[c] + sum_{dy, dx, ci} w[c, ci, dy, dx] * f[b, py - 1 + dy, px - 1 + dx, ci]),
 *   (py, px) = (2 y_id + k [t & 1], 2 x_id + k [t >> 1]),  t = 0..3 in the reference's sf1..sf4 order.
 * f (B, H, W, in_cstride) channels [in_coff, +256); w fp32 (64, 256, 2, 2) packed by cp_pack_index2feat_conv_weight into
 * cp_index2feat_conv_weight_bytes() bytes; out (B, N, out_cstride) channels [out_coff, +256).  Used where it is cheaper than
 * cp_conv2d_igemm + cp_index2feat_gather (the 64 x 64 stage at N = 512: half the FLOPs, no (H+1) x (W+1) x 64 tensor). */
int cp_index2feat_conv_supported(int Cin, int E_ch, int k);
size_t cp_index2feat_conv_weight_bytes(void);
int cp_pack_index2feat_conv_weight(cp_stream_t stream, const float* w, void* packed);
int cp_index2feat_conv(cp_stream_t stream, const void* f, int in_cstride, int in_coff, const void* packed_w, const float* bias,
                       const int32_t* x_id, const int32_t* y_id, const float* mask, void* out, int B, int N, int H, int W, int k,
                       int out_cstride, int out_coff);
/* ... the (bf16) conv's output rows written as `out_dtype` = CP_BF16 or CP_F16 */
int cp_index2feat_conv_t(cp_stream_t stream, int out_dtype, const void* f, int in_cstride, int in_coff, const void* packed_w,
                         const float* bias, const int32_t* x_id, const int32_t* y_id, const float* mask, void* out, int B, int N,
                         int H, int W, int k, int out_cstride, int out_coff);

/* Bit decode (pipeline.py:72-127, 367-369, 380-381) on the fp32 logit block `bits` (B, 13, N):
 * row 0 = roi, rows 1..6 = x bits (MSB first), rows 7..12 = y bits.
 *   stage < 0 : mask = bit(bits[0]) ; x_id = MSB-first int of rows 1..3 ; y_id of rows 7..9
 *   stage = i : x_id = 2*x_id + bit(bits[4+i]) ; y_id = 2*y_id + bit(bits[10+i])
 * bit(z) = [sigmoid(z) > 0.5 in fp32] = [z > CP_SIGMOID_HALF_Z0]: fp32 sigmoid is exactly 0.5 on 0 <= z <= 1.5 * 2^-24
 * (measured through the reference's from_mask_prob_to_mask; fixture tests/golden/sigmoid_threshold.npz), so `z > 0`
 * would differ from the reference there.  Also mirrors the ids to int64 (the reference's return dtype). */
#define CP_SIGMOID_HALF_Z0_BITS 0x33C00000u   /* largest fp32 z with sigmoidf(z) == 0.5f: 8.940696716e-08 */
int cp_bits_decode(cp_stream_t stream, const float* bits, int stage, float* mask, int32_t* x_id,
                   int32_t* y_id, int64_t* x_id64, int64_t* y_id64, int B, int N);
/* Code decode of a block that holds one head's rows packed (the woProg ablation, pipeline_lm.py:511-516): rows 1..r of
 * bits (B, rows, N) are the x code, rows r+1..2r the y code, MSB first; x_id64 / y_id64 (B, N) int64 required, x_id32 / y_id32
 * optional; 1 <= r, 1 + 2r <= rows.  The same bit predicate as cp_bits_decode (and cp_mlp_query_fused_n's epilogue). */
int cp_code_decode(cp_stream_t stream, const float* bits, int rows, int r, int64_t* x_id64, int64_t* y_id64, int32_t* x_id32,
                   int32_t* y_id32, int B, int N);

/* Post-forward decode on the device (next-row N2; reference test.py:294-329 + test_network_with_test_data.py:50-66):
 * bits (B,13,N) fp32 logits, seg (B,2,H,W) fp32 logits (0 = visible, 1 = full), ids int64 (B,N), roi_xy_ori (B,2,H,W)
 * fp32 -> p2d (B,N,2) fp32, valid (B,N,3) uint8 [all | full-mask | visible-mask], count (B,3) int32.
 * discard_bd_pixel = from_id_to_pose's argument of that name (:60-63): d > 0 drops keypoints whose pixel lies within d
 * pixels of the RoI border (d <= x < W-d, d <= y < H-d must hold); 0 = off (the reference's default). */
int cp_correspondences(cp_stream_t stream, const float* bits, const float* seg, const int64_t* x_id, const int64_t* y_id,
                       const float* roi_xy_ori, float* p2d, uint8_t* valid, int32_t* count, int B, int N, int H, int W,
                       int discard_bd_pixel);
/* The same with the coordinate grid built on the fly from the crop's final box (device, B x 4 int32: x, y, w, h = get_final_Bbox,
 * bop_dataset_pytorch.py:188-222) instead of a (B,2,H,W) roi_xy_ori tensor uploaded per batch: p2d = (float)(w / W * x_id + x) etc.
 * in fp64 then fp32, exactly the entries of the loader's grid (mapping_pixel_position_to_original_position_2d :223-235, :380). */
int cp_correspondences_bbox(cp_stream_t stream, const float* bits, const float* seg, const int64_t* x_id, const int64_t* y_id,
                            const int32_t* final_bbox, float* p2d, uint8_t* valid, int32_t* count, int B, int N, int H, int W,
                            int discard_bd_pixel);

/* Pose from the correspondences, on the device (next-row N4; reference test_network_with_test_data.py:100-114: the call
 *   cv2.solvePnPRansac(valid_p3d, valid_disc_p2d, cam_K, None, reprojectionError, iterationsCount, flags=cv2.SOLVEPNP_EPNP)
 * and the identity-pose fallback below 4 valid correspondences), one workgroup per crop, fp64 arithmetic:
 *   p3d fp32 (N,3) model keypoints in their ORIGINAL units (batch stride p3d_bstride elements; 0 = one object for all crops);
 *   p2d fp32 (B,N,2) and valid uint8 with `valid_stride` bytes between keypoints = cp_correspondences' outputs (valid + column c,
 *   stride 3: c = 0 all | 1 in full mask | 2 in visible mask);  cam_K fp32 row-major 3x3 (batch stride K_bstride; 0 = shared);
 *   RANSAC over `iterations` (<= 256) EPnP hypotheses of 5 correspondences drawn by a counter-based
 *   hash of (seed, crop, hypothesis), inlier test squared reprojection error <= reproj_threshold^2, the hypothesis with the most
 *   inliers (>= the sample size; first on ties), final EPnP over its inliers.  Exactly 4 valid correspondences: no RANSAC, as in
 *   OpenCV (model_points == npoints) -- P3P on the first three, the fourth picks among the up-to-four poses, all four are inliers.
 * Outputs: pose fp64 (B,12) = [R row-major | t], inliers uint8 (B,N), status int32 (B): 1 = solved, 0 = identity fallback.
 * scratch: cp_pnp_ransac_scratch_bytes(B, N) bytes, 8-byte aligned.  What the call leaves in it is part of the interface (the tests
 *   replay the solver's decisions from it): one record of 14 doubles per hypothesis h of crop b at (b * iterations + h) * 14 --
 *   [0] the inlier count of the hypothesis' pose among the valid correspondences, or -1 when its sample gave no pose (degenerate);
 *   [1] unused, never written; [2..10] R row-major and [11..13] t, written only when [0] >= 0.  Hypotheses run in rounds of 64;
 *   the records of a round that OpenCV's stopping rule (RANSACUpdateNumIters, confidence 0.99, on the best count of the earlier
 *   rounds) cuts off are not written, nor is any record of a crop with fewer than 5 valid correspondences; bytes behind
 *   B * iterations records are never touched.  A caller that wants to tell written records apart fills the scratch first.
 * opencv-python is not part of the reference's tree: the algorithm is restated from
 * the publication / OpenCV's structure (oracle/pnp_oracle.py lists the deliberate differences); parity with cv2 is UNPINNED. */
size_t cp_pnp_ransac_scratch_bytes(int B, int N);
int cp_pnp_ransac(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
                  int valid_stride, const float* cam_K, long long K_bstride, int B, int N, float reproj_threshold,
                  int iterations, uint32_t seed, double* pose, uint8_t* inliers, int32_t* status, void* scratch);

/* Graph-cut RANSAC pose solver (row N17): what the reference's `--use_progressivex` path (pyprogressivex.find6DPoses,
 * test_network_with_test_data.py:68-99) comes down to with maximum_model_number = 1 -- RANSAC from a minimal solver, a locally
 * optimised model whose inlier set is a two-label graph cut over a neighbourhood graph, a refit over that labelling repeated while
 * it improves.  pyprogressivex is not part of the reference's tree: the rule is this project's own (tests/gc_stages.py restates
 * it in numpy); parity with pyprogressivex -- its sampler, confidence default, unary kernel, inner RANSAC, neighbourhood space and
 * PEARL's model validation -- is UNPINNED.
 *
 * cp_radius_graph_count / _fill: the neighbourhood graphs of M objects of N (<= 4096) fp32 keypoints each, pts (M,N,3): pair {i,j},
 *   i != j, is an edge when dx*dx + dy*dy + dz*dz <= radius^2, evaluated in fp64 from the fp32 coordinates without contraction
 *   (MODEL space: static per object and symmetric; which space pyprogressivex's FLANN graph lives in cannot be checked).
 *   count writes offsets int32 (M,N+1) -- the CSR row starts of object m RELATIVE to that object's first edge -- and totals int32
 *   (M) = directed edges per object.  The caller reads the totals, refuses more than 2^21 per object, forms base int64 (M) = the
 *   exclusive prefix sums of the totals and calls fill, which writes indices int32 [n_indices] (n_indices = sum of the totals):
 *   the neighbours of keypoint i of object m at base[m] + offsets[m][i] ..., ascending.
 * cp_graphcut_label: the labelling alone, B problems over ONE graph (offsets (N+1), indices [n_edges], symmetric, columns ascending):
 *   cin int32 (B,N), -1 = not a node.  Network: s->i = Q = 65536, i->t = cin_i, i<->j = w per direction on every edge between two
 *   nodes.  labels uint8 (B,N) = the MINIMAL source side of a minimum cut (unique, whatever the maximum flow), flow_value int64 (B)
 *   = the value of the maximum flow, status int32 (B): 0, or -1 when the bounded number of push-relabel sweeps did not suffice
 *   (labels 0, flow_value -1: never an approximate labelling); sweeps int32 (B) or NULL: sweeps run (the one
 *   output that depends on thread timing).  scratch: at least
 *   B * max(n_edges, 1) * 4 bytes (`scratch_bytes` says how many there are).  0 <= w <= 2^28.
 * cp_pnp_gc: inputs and outputs as cp_pnp_ransac; the graph of crop b is object graph_ids[b] (NULL: object 0; required when M > 1),
 *   max_edges = the largest total of any object, w = floor(spatial_coherence_weight * 65536 + 0.5), iterations in 1..512,
 *   min_inliers >= 4.  Per crop: hypotheses in rounds of 64 -- hypothesis h draws 4 distinct valid correspondences by the hash of
 *   (seed, crop, h), P3P on three, the fourth picks the root; count = valid points with r^2 <= thr^2, score = sum of 1 - r^2/thr^2
 *   over them (MSAC); OpenCV's stopping rule on the counts between rounds (sample size 4).  Winner P_0 = the first record with the
 *   largest score among those with count >= 4.  Step k = 0..8: cin_i = floor(min(r_i^2/thr^2, 2^14) * 65536 + 0.5) under P_k,
 *   L_k = the labelling above; stop if |L_k| < min_inliers; for k < 8: Q_k = EPnP over L_k (cp_pnp_ransac's refit), stop if it
 *   fails or score(Q_k) <= score(P_k), else P_{k+1} = Q_k.  Returned: the last P_k and L_k with status 1 when |L_k| >= min_inliers,
 *   else the identity with status 0 (also with fewer than min_inliers valid points or no record with count >= 4).  status -1: the
 *   sweep bound was hit, -2: graph_ids[b] / base outside the graph (identity pose, no inliers either way).
 *   scratch: cp_pnp_gc_scratch_bytes(B, N, max_edges) bytes (0 = bad arguments), 8-byte aligned; what the call leaves is part of the
 *   interface, at byte offsets: 0: hypothesis records, 14 doubles at (b * iterations + h) * 14 = [count or -1, score, R, t] (score
 *   and pose only when count >= 0; unwritten as in cp_pnp_ransac); B*512*14*8: step records, 30 doubles at (b * 9 + k) * 30 =
 *   [k, P_k (12), score(P_k), |L_k|, refit 1 / 0, Q_k (12), score(Q_k), sweeps (timing-dependent)], a word written only when its stage ran; then
 *   cin int32 (B,9,N), then labels uint8 (B,9,N), then (8-byte aligned) the flows. */
int cp_radius_graph_count(cp_stream_t stream, const float* pts, int M, int N, double radius, int32_t* offsets, int32_t* totals);
int cp_radius_graph_fill(cp_stream_t stream, const float* pts, int M, int N, double radius, const int32_t* offsets,
                         const int64_t* base, int32_t* indices, long long n_indices);
int cp_graphcut_label(cp_stream_t stream, const int32_t* cin, const int32_t* offsets, const int32_t* indices, int B, int N,
                      long long n_edges, int32_t w, uint8_t* labels, int64_t* flow_value, int32_t* status, int32_t* sweeps,
                      void* scratch, size_t scratch_bytes);
size_t cp_pnp_gc_scratch_bytes(int B, int N, long long max_edges);
int cp_pnp_gc(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
              int valid_stride, const float* cam_K, long long K_bstride, const int32_t* g_offsets, const int32_t* g_indices,
              const int64_t* g_base, const int32_t* graph_ids, int M, long long max_edges, long long n_indices, int B, int N,
              float reproj_threshold, int32_t w, int iterations, int min_inliers, uint32_t seed, double* pose,
              uint8_t* inliers, int32_t* status, void* scratch);

/* Levenberg-Marquardt polish of solved poses (row N22): the non-linear refinement of the reprojection error over a crop's selected
 * correspondences -- the inliers of cp_pnp_ransac or cp_pnp_gc -- that a cv2 user gets from solvePnPRefineLM.  The reference does not
 * refine; opt-in, the rule is this project's own (stated in full at the top of csrc/pnp_refine.hip, restated in numpy by
 * tests/lm_stages.py); parity with cv2 is UNPINNED.  One launch, one workgroup per crop, fp64 without contraction.
 *   p3d, p3d_bstride, p2d, cam_K, K_bstride, B, N as cp_pnp_ransac (N <= 4096; B == 0 returns without a launch);
 *   mask uint8, `mask_stride` bytes between keypoints, (b * N + i) * mask_stride: non-zero = selected;
 *   pose_in fp64 (B,12) = [R row-major | t]; status_in int32 (B) or NULL: 0 = leave this crop's pose alone;
 *   max_iters in 1..64; step_tol > 0, finite.
 * Per crop: cost c = sum of squared reprojection errors (pixels^2) over the n selected points; increment d = (w, v) with
 *   R' = exp([w]x) R, t' = t + v; H = sum J^T J, g = sum J^T r.  lambda = 1e-3; an iteration solves (H + lambda diag H) d = -g by
 *   Cholesky (not positive definite: rejected, c' = +inf, d NaN), accepts iff c' < c (c' = +inf when a selected point is not in front
 *   of the camera or c' is not finite), then lambda = max(lambda / 10, 1e-12) or lambda * 10; s = max(|w|_inf, |v|_inf / |t|).
 *   Stops: s <= step_tol -> status 1; lambda > 1e8 after a rejection -> 3; max_iters iterations -> 2.
 *   Status 0 = pass-through, pose_out BITWISE pose_in: status_in 0, n < 6, a non-finite input pose or selected pixel, a selected
 *   point with C_z <= 0 under the input pose.
 * Outputs: pose_out fp64 (B,12) (bitwise the last accepted trial, or pose_in; pose_out == pose_in is allowed, a partial overlap is
 *   refused), status_out int32 (B), info fp64 (B, cp_pnp_refine_lm_info_doubles() = 40) = [c at the input pose, c at the returned
 *   pose, n, iterations run, the undamped H at the returned pose (36, row-major; order w then v)] (status 0: NaN but for n and 0
 *   iterations); records fp64 (B, max_iters, cp_pnp_refine_lm_record_doubles() = 17) or NULL: per executed iteration [lambda used,
 *   c, c', accepted 0/1, s, R' (9), t' (3)]; slots of iterations that did not run are never written (a caller that wants to tell
 *   them apart fills the buffer first). */
int cp_pnp_refine_lm_record_doubles(void);
int cp_pnp_refine_lm_info_doubles(void);
int cp_pnp_refine_lm(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* mask,
                     int mask_stride, const float* cam_K, long long K_bstride, int B, int N, const double* pose_in,
                     const int32_t* status_in, int max_iters, double step_tol, double* pose_out, int32_t* status_out,
                     double* info, double* records);

/* Per-keypoint, per-axis pixel variance of the decoded code from the code logits' confidences (row N32; opt-in, the rule is this
 * project's own: stated in full at the top of csrc/code_confidence.hip, restated in numpy by tests/wlm_stages.py).
 *   bits (B, rows, N) fp32 as cp_code_decode reads it: row 0 the RoI bit, rows 1..r the x bits MSB first, rows 1+r..2r the y bits,
 *   1 <= r <= 30, rows >= 1 + 2r; final_bbox (B,4) int32 (x, y, w, h) as cp_correspondences_bbox reads it; the code grid (Hc, Wc);
 *   floor_cells2 > 0, finite: the variance floor in cells^2 (1/12 = uniform quantisation to one cell).
 * Per bit with logit z: e = exp(-|z|), q = e / ((1 + e)(1 + e)) = p (1 - p); per axis v = sum_j 4^(r-1-j) q_j (j = 0 the MSB, summed
 * ascending): the variance of the code under independent Bernoulli bits.  sigma2 fp64 (B,N,2) = [(w / Wc)^2 (floor + v_x),
 * (h / Hc)^2 (floor + v_y)] in pixels^2, fp64 without contraction; 0 on an axis whose box side is 0; NaN where a logit is NaN.
 * One launch, one lane per (crop, keypoint); B == 0 returns without a launch.  Whether a trained network's logits are calibrated
 * enough for v to be a variance in fact is UNPINNED. */
int cp_code_confidence(cp_stream_t stream, const float* bits, int rows, int r, const int32_t* final_bbox, int B, int N, int Hc, int Wc,
                       double floor_cells2, double* sigma2);

/* Weighted robust Levenberg-Marquardt polish of solved poses (row N32): cp_pnp_refine_lm with a per-point, per-axis scale on the
 * residuals and a Huber loss (stated in full at the top of csrc/pnp_refine_w.hip, restated in numpy by tests/wlm_stages.py).
 * Arguments, refusals, statuses, records (17 doubles) and the returned pose as cp_pnp_refine_lm, plus
 *   scale fp32 (B,N,2) = 1 / sigma per axis (e.g. rsqrt of cp_code_confidence's sigma2): whitened components u = scale * r, Jacobian
 *   rows scaled alike, the scale applied before any product (a scale of exactly 1 changes no operand); a NULL scale is refused;
 *   huber_delta > 0 in whitened units, +inf allowed (the unrobust fit), NaN or <= 0 refused: per scalar component
 *   rho(u) = u^2 if |u| <= delta else 2 delta |u| - delta^2, weight omega = 1 or delta / |u|; cost c = sum rho; H = sum omega j j^T,
 *   g = sum omega u j (half the gradient of c); accept iff c' < c on this cost.
 * Status 0 (pass-through, pose_out BITWISE pose_in) under cp_pnp_refine_lm's conditions, plus a selected point whose scale is not
 * finite or <= 0.  info fp64 (B, cp_pnp_refine_wlm_info_doubles() = 42): cp_pnp_refine_lm's 40 (H = the whitened, omega-weighted
 * matrix at the returned pose: its inverse is the covariance), then the number of components with |u| > delta at the input pose,
 * then at the returned pose. */
int cp_pnp_refine_wlm_info_doubles(void);
int cp_pnp_refine_wlm(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* mask,
                      int mask_stride, const float* scale, const float* cam_K, long long K_bstride, int B, int N, const double* pose_in,
                      const int32_t* status_in, double huber_delta, int max_iters, double step_tol, double* pose_out,
                      int32_t* status_out, double* info, double* records);

/* Confidence-guided pose solver (row N33): cp_pnp_ransac fed with cp_code_confidence's variances -- the correspondences ranked by
 * variance, 5-point samples drawn PROSAC-style from a pool that grows down the ranking, inliers gated on the whitened residual.  Opt-in,
 * the rule is this project's own (stated in full at the top of csrc/pnp_conf.hip, restated in numpy by tests/cpnp_stages.py).
 * cp_rank_correspondences: sigma2 fp64 (B,N,2) pixels^2 (x, y), 8-byte aligned; valid / valid_stride as cp_pnp_ransac.  A valid keypoint
 *   is ranked iff both variances are finite and > 0; key = sigma2_x + sigma2_y (one fp64 add); order int32 (B,N) = the ranked keypoints
 *   by ascending key, ties by ascending index, -1 beyond n_ranked[b]; n_dropped[b] = the valid keypoints that are not ranked.  One
 *   launch, one workgroup per crop (bitonic sort in LDS), N <= 4096; B == 0 returns without a launch.
 * cp_pnp_conf: p3d .. N, iterations, seed, pose, inliers, status as cp_pnp_ransac (the same refusals), plus sigma2 as above,
 *   chi2_threshold finite and > 0 (refused otherwise; 5.99 / 9.21 = the 95 % / 99 % quantiles of chi^2 with 2 degrees of freedom),
 *   guided (0: every sample drawn from all ranked points), and the ranking's three outputs, which the call fills first (required).
 *   Hypothesis h draws its sample from the first n_h of the ranking, n_h = the smallest n in [5, nv] with
 *   C(n,5) * iterations >= (h + 1) * C(nv,5) in exact integers (nv = n_ranked); keypoint i is an inlier iff
 *   du^2 / sigma2_x + dv^2 / sigma2_y <= chi2_threshold (fp64, no contraction); dropped keypoints are never sampled and never inliers.
 *   Rounds, stopping rule, winner, unweighted EPnP refit over the winner's inliers, P3P at nv == 4, identity below: as cp_pnp_ransac.
 * scratch: cp_pnp_conf_scratch_bytes(B, N) bytes, 8-byte aligned: cp_pnp_ransac's records, [1] = n_h (written with every record). */
int cp_rank_correspondences(cp_stream_t stream, const double* sigma2, const uint8_t* valid, int valid_stride, int B, int N,
                            int32_t* order, int32_t* n_ranked, int32_t* n_dropped);
size_t cp_pnp_conf_scratch_bytes(int B, int N);
int cp_pnp_conf(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid, int valid_stride,
                const double* sigma2, const float* cam_K, long long K_bstride, int B, int N, double chi2_threshold, int iterations,
                uint32_t seed, int guided, double* pose, uint8_t* inliers, int32_t* status, int32_t* order, int32_t* n_ranked,
                int32_t* n_dropped, void* scratch);

/* Calibration of the code logits (row N34): the instrument behind rows N32 / N33, which read the logits as probabilities.  Opt-in, the
 * rule is this project's own (stated in full at the top of csrc/calibrate.hip -- the order of every floating sum included -- and
 * restated in numpy by tests/calib_stages.py).  fp64 without contraction, no global atomics: integer outputs do not depend on the launch
 * shape, two calls agree bitwise.
 * Shared arguments: bits (B, rows, N) fp32 logits with `bits_bstride` elements between crops (>= rows * N), row 0 the RoI bit, rows
 *   1..r the x bits MSB first, rows 1+r..2r the y bits, 1 <= r <= 30, rows >= 1 + 2r (K = 1 + 2r rows are read); gt_roi (B,1,N), gt_x /
 *   gt_y (B,gt_bits,N) fp32 with gt_bits >= r: cp_encode_targets' labels (set iff > 0.5).  Row 0 counts every (b, n), the x / y rows only
 *   where the GT RoI bit is set; a NaN logit is counted in n_nan alone.  B == 0 returns CP_OK without a launch (outputs untouched).
 * cp_code_reliability: scale_host (K) fp64 in HOST memory, each finite and > 0: t = (double)z * scale[k]; edges_host (M - 1) fp64 in HOST
 *   memory, no NaN, strictly ascending, in LOGIT space, 1 <= M <= 64 (NULL allowed at M == 1): bin = the number of edges <= t.
 *   p = sigmoid(t) and nll in the overflow-free forms of the kernel file.  Outputs on the device, 8-byte aligned:
 *   ints int64 (K, 2M + 3) = [count per bin | positives per bin | n | n_nan | n_right = samples with (z > 0) == y], sums fp64 (K, M + 4) = [sum_p per bin | nll | brier |
 *   g = sum (p - y) z | h = sum p (1 - p) z^2].  scratch: cp_code_reliability_scratch_bytes(r, M) bytes, 8-byte aligned (0 = bad
 *   arguments).  Two launches: 1024 workgroups over contiguous slices of (b, n), then one workgroup that adds their records in order.
 * cp_fit_code_scale: group_of_row_host (K) int32 in HOST memory, values in [0, n_groups), 1 <= n_groups <= K: every group minimises its
 *   rows' summed nll over one shared s by the bracketed Newton iteration of the kernel file: s = 1, bracket [s_min, s_max] with
 *   0 < s_min <= 1 <= s_max finite and s_min < s_max, step_tol finite > 0, 1 <= max_iters <= CP_CALIB_MAX_ITERS evaluations, then one
 *   more at the returned s.  1 + 2 (max_iters + 1) launches are enqueued at once, nothing synchronises; a stopped group is frozen.
 *   scale fp64 (K): the row's group's s; info fp64 (n_groups, cp_fit_code_scale_info_doubles() = 12): s, lo, hi, status (CP_CALIB_*),
 *   evaluations, nll_before (at s = 1), nll_after (at the returned s), n, then four internal words.  scratch:
 *   cp_fit_code_scale_scratch_bytes(r) bytes, 8-byte aligned.
 * cp_sigma2_consistency: p2d fp32 (B,N,2); proj_xy fp64 (B,N,2) (cp_encode_targets); sigma2 fp64 (B,N,2) (cp_code_confidence); valid /
 *   valid_stride as cp_pnp_conf; gt_roi (B,1,N); edges_host (E) fp64 in HOST memory, no NaN, strictly ascending, chi-square units,
 *   0 <= E <= 63.  Point n counts iff valid, GT RoI set and both variances finite and > 0.  d2 = du^2 / sigma2_x + dv^2 / sigma2_y with
 *   du = (double)p2d_x - proj_x; bin = the number of edges <= d2.  counts int32 (B, E + 1); n_counted_dropped int32 (B,2); sums fp64
 *   (B,3) = sum d2, sum du / sqrt(sigma2_x), sum dv / sqrt(sigma2_y).  One launch, one workgroup per crop: a crop's outputs do not
 *   depend on the batch it is in. */
#define CP_CALIB_OK 0
#define CP_CALIB_CAPPED_HIGH 1      /* the bracket collapsed onto s_max and g(s_max) < 0: every sign is right */
#define CP_CALIB_CAPPED_LOW 2       /* ... onto s_min and g(s_min) > 0 */
#define CP_CALIB_EMPTY 3            /* no counted sample: s stays 1 */
#define CP_CALIB_NOT_CONVERGED 4    /* max_iters evaluations without a step <= step_tol * s: s = the evaluated point of the lowest nll */
#define CP_CALIB_MAX_ITERS 256
size_t cp_code_reliability_scratch_bytes(int r, int M);
int cp_code_reliability(cp_stream_t stream, const float* bits, long long bits_bstride, int rows, int r, const float* gt_roi,
                        const float* gt_x, const float* gt_y, int gt_bits, const double* scale_host, const double* edges_host, int M,
                        int B, int N, long long* ints, double* sums, void* scratch);
int cp_fit_code_scale_info_doubles(void);
size_t cp_fit_code_scale_scratch_bytes(int r);
int cp_fit_code_scale(cp_stream_t stream, const float* bits, long long bits_bstride, int rows, int r, const float* gt_roi,
                      const float* gt_x, const float* gt_y, int gt_bits, const int32_t* group_of_row_host, int n_groups, int B, int N,
                      double s_min, double s_max, double step_tol, int max_iters, double* scale, double* info, void* scratch);
int cp_sigma2_consistency(cp_stream_t stream, const float* p2d, const double* proj_xy, const double* sigma2, const uint8_t* valid,
                          int valid_stride, const float* gt_roi, const double* edges_host, int E, int B, int N, int32_t* counts,
                          int32_t* n_counted_dropped, double* sums);

/* Projective point-to-plane ICP of poses against a depth image (row N24): the depth refinement of an RGB-only pose.  The reference
 * does not refine; opt-in, the rule is this project's own (stated in full at the top of csrc/icp_refine.hip, restated in numpy by
 * tests/icp_stages.py); parity with any ICP library is UNPINNED.
 * cp_surface_samples (stage A): one raster pass of P poses (poses, cam_K, k_stride, verts .. Vmax, H, W as cp_render_depth), then per
 *   pose a lattice of at most grid x grid (grid in 1..64) pixels over its vertex rectangle inside the frame; S = grid * grid slots.
 *   Outputs: rect int32 (P,4) x0 y0 x1 y1 (-1 four times when empty), shape int32 (P,2) nx ny, pixel int32 (P,S,2) (-1 -1 beyond
 *   nx * ny), depth fp32 (P,S) (cp_render_depth's bits at the pixel, 0 = not covered), face int32 (P,S) (-1 = empty slot), X, N fp64
 *   (P,S,3) the sample's model-space point and unit face normal towards the camera (NaN in an empty slot), ok int32 (P) (0: not
 *   rendered).  scratch: cp_surface_samples_scratch_bytes(P, Vmax) bytes, 16-byte aligned.  Four launches, no atomics but the
 *   scaffold's integer rectangle merge.
 * cp_icp_refine (stages B and C): ONE launch, one workgroup per pose, fp64 without contraction.
 *   pose_in fp64 (P,12) = [R row-major | t]; cam_K fp64 with k_stride 0 or 9; X, N, face: cp_surface_samples' outputs with S slots per
 *   pose (1..4096); depth fp32 (I,H,W) the sensor's images, image_ids int32 (P) or NULL with I == 1; max_dist fp64 (P); diameters fp64
 *   (M) with mesh_ids int32 (P) or NULL with M == 1 (rho = diameter / 2); status_in int32 (P) or NULL: 0 = leave this pose alone;
 *   max_iters in 1..64; step_tol > 0, finite; min_pairs >= 6; inertia >= 0, finite.
 *   Outputs: pose_out fp64 (P,12) (bitwise the last accepted trial, or pose_in; pose_out == pose_in is allowed, a partial overlap is
 *   refused); status_out int32 (P): 1 step rule, 2 max_iters, 3 lambda > 1e8 or fewer than min_pairs pairs after a step, 0 =
 *   pass-through; info fp64 (P, cp_icp_refine_info_doubles() = 42) = [c at the input pose, c at the returned pose, samples, pairs at
 *   the input pose, pairs at the returned pose, iterations, undamped H at the returned pose (36; w then v)] (status 0: NaN but for
 *   the counts); records fp64 (P, max_iters, cp_icp_refine_record_doubles() = 18) or NULL: per executed iteration [lambda used, n, c,
 *   c', accepted 0/1, s, R' (9), t' (3)]; slots of iterations that did not run are never written.
 * CP_ERR_INVALID: a null pointer, the mesh / view / image argument rules of the raster family, a grid, S, max_iters, step_tol,
 * min_pairs or inertia outside its range, a partial overlap of the poses; CP_ERR_ALIGN; CP_ERR_RANGE: H * W >= 2^31, too many blocks. */
size_t cp_surface_samples_scratch_bytes(int P, int Vmax);
int cp_surface_samples(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                       const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                       int H, int W, int P, int Vmax, int grid, int32_t* rect, int32_t* shape, int32_t* pixel, float* depth,
                       int32_t* face, double* X, double* N, int32_t* ok, void* scratch);
int cp_icp_refine_record_doubles(void);
int cp_icp_refine_info_doubles(void);
int cp_icp_refine(cp_stream_t stream, const double* pose_in, const double* cam_K, int k_stride, const double* X, const double* N,
                  const int32_t* face, int S, const float* depth, const int32_t* image_ids, int I, int H, int W,
                  const double* max_dist, const double* diameters, int M, const int32_t* mesh_ids, const int32_t* status_in,
                  int max_iters, double step_tol, int min_pairs, double inertia, int P, double* pose_out, int32_t* status_out,
                  double* info, double* records);

/* Pose from depth-lifted correspondences (row N25): RANSAC over three-pair absolute orientation with a local optimisation, for an
 * RGB-D frame resident on the device.  The reference uses no depth at test time; opt-in, the rule is this project's own (stated in
 * full at the top of csrc/pose_depth.hip, restated in numpy by tests/depth_pose_stages.py); parity with any library is UNPINNED.
 *   p3d, p3d_bstride, p2d, valid, valid_stride, cam_K (fp32), K_bstride, B, N, seed, pose, inliers, status as cp_pnp_ransac
 *   (N <= 4096; B == 0 returns without a launch); depth fp32 (I,H,W) the sensor's images in the keypoints' units; image_ids int32 (B)
 *   names each crop's image, NULL = image 0 for all when I == 1, image b for crop b when I == B (anything else is refused); an id
 *   outside 0..I-1 lifts nothing.
 * cp_lift_correspondences (stage A; one memset and one launch): a valid keypoint with (u, v) = its p2d reads z = depth[image, floor v,
 *   floor u]; it is dropped outside the frame or when z is not finite or <= 0, else Q = ((u - cx) / fx z, (v - cy) / fy z, z) in fp64,
 *   rounded once.  Q fp32 (B,N,3) (0 where dropped), lifted uint8 (B,N), n_lifted int32 (B).
 * cp_pose_depth_ransac (stage A into the scratch, then ONE launch, one workgroup per crop, fp64 without contraction): over the n
 *   lifted keypoints, hypotheses from 3 distinct positions (the hash sampler of cp_pnp_ransac with m = 3) in rounds of 64 with OpenCV's
 *   stopping rule between them (sample size 3); a sample whose model points are collinear (|e1 x e2|^2 <= 1e-12 (max squared edge)^2) or
 *   whose cross-covariance has rank < 2 is degenerate; inliers: |R X + t - Q|^2 <= threshold^2; the winner has the most inliers (>= 3),
 *   first on ties; then the least-squares pose over its inliers, re-evaluated at most 3 times while the inlier set grows.  n < 3, no
 *   winner, or a per-crop threshold that is not positive and finite: the identity with status 0 and no inliers.
 *   dist_thresholds fp64 (B) on the device or NULL = dist_threshold (a number, positive and finite) for all; iterations in 1..256.
 *   scratch: cp_pose_depth_ransac_scratch_bytes(B, N, iterations) bytes (0 = bad arguments), 8-byte aligned; what the call leaves is
 *   part of the interface, at byte offsets: 0: hypothesis records, cp_pose_depth_record_doubles() = 14 doubles at (b * iterations + h)
 *   * 14 = [count or -1, unused and never written, R row-major, t] (pose only when count >= 0; records of rounds the stopping rule cut
 *   off, and of crops that fell back before the rounds, unwritten); B*iterations*14*8: 4 step records of 14 doubles per crop = [the
 *   step's inlier count, accepted 0/1, R, t of the state after the step] (step 0: the first fit; unwritten where none ran); then Q fp32
 *   (B,N,3), n_lifted int32 (B), lifted uint8 (B,N): stage A's outputs.
 * CP_ERR_INVALID: a null pointer, a size, stride, iteration count or threshold outside its range, several images without ids;
 * CP_ERR_ALIGN; CP_ERR_RANGE: H * W >= 2^31, B >= 2^24. */
int cp_lift_correspondences(cp_stream_t stream, const float* p2d, const uint8_t* valid, int valid_stride, const float* cam_K,
                            long long K_bstride, const float* depth, const int32_t* image_ids, int I, int H, int W, int B, int N,
                            float* Q, uint8_t* lifted, int32_t* n_lifted);
size_t cp_pose_depth_ransac_scratch_bytes(int B, int N, int iterations);
int cp_pose_depth_record_doubles(void);
int cp_pose_depth_ransac(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
                         int valid_stride, const float* cam_K, long long K_bstride, const float* depth, const int32_t* image_ids,
                         int I, int H, int W, int B, int N, double dist_threshold, const double* dist_thresholds, int iterations,
                         uint32_t seed, double* pose, uint8_t* inliers, int32_t* status, void* scratch);

/* Hypothesis verification of poses against a depth image, and the choice among candidates (row N26).  The reference does not verify;
 * opt-in, the rule is this project's own (stated in full at the top of csrc/pose_verify.hip, restated in numpy by
 * tests/verify_stages.py).
 * cp_verify_poses: P poses (poses, cam_K, k_stride, verts .. Vmax, H, W as cp_render_depth; depth, image_ids, I as cp_gt_info) are
 *   rendered tile by tile -- no depth frame is stored -- and every model pixel (render D > 0) is classified against the sensor depth S
 *   with the pose's tolerance tau (fp64 (P) on the device, converted to fp32 once): missing (S not finite or <= 0), match
 *   (|S - D| <= tau, which also adds q = min(63, (int)(64 (|S - D| / tau))) to sum_q), occluded (S - D < -tau), through (S - D > tau).
 *   status int32 (P) or NULL: a pose whose entry is 0 is not a candidate.  occlusion_weight in [0, 1].
 *   Outputs: counts int32 (P,6) = n_model n_missing n_match n_occluded n_through sum_q; fit = n_match - sum_q / 64, den = n_match +
 *   n_through + occlusion_weight n_occluded, score = fit / den, all fp64 (P); ok uint8 (P).  score is NaN with ok = 0 when den == 0 or
 *   the pose is not counted (all six counts 0): a non-finite pose or cam_K, a vertex at Z <= 0, an image or mesh id out of range,
 *   status 0, a tau that as fp32 is not positive and finite.  labels uint8 (P,H,W) or NULL: 0 none, 1 match, 2 occluded, 3 through,
 *   4 missing.  scratch: cp_verify_poses_scratch_bytes(P, Vmax) bytes (0 = bad arguments), 16-byte aligned.  Four launches; every
 *   output is a function of integer sums: bitwise the same alone or in a batch, with or without labels.
 * cp_select_poses: score fp64 (C,B) candidate-major, ok uint8 (C,B) or NULL (then every score that is not NaN is eligible), C in 1..64
 *   -> choice int32 (B): the eligible candidate with the largest score, the smallest index on equal scores, 0 when none is eligible.
 * CP_ERR_INVALID: a null pointer, the mesh / view / image argument rules of the raster family, an occlusion_weight outside [0, 1], C
 * or B outside its range; CP_ERR_ALIGN; CP_ERR_RANGE: H * W > 2^24 (the sums are int32), too many blocks, C * B >= 2^31. */
size_t cp_verify_poses_scratch_bytes(int P, int Vmax);
int cp_verify_poses(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                    const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                    const float* depth, const int32_t* image_ids, int I, int H, int W, const double* tau, const int32_t* status,
                    double occlusion_weight, int P, int Vmax, int32_t* counts, double* score, double* fit, double* den, uint8_t* ok,
                    uint8_t* labels, void* scratch);
int cp_select_poses(cp_stream_t stream, const double* score, const uint8_t* ok, int C, int B, int32_t* choice);

/* Hypothesis verification of poses against predicted masks (row N28): row N26 for RGB-only data.  The reference does not verify;
 * opt-in, the rule is this project's own (stated in full at the top of csrc/pose_verify_mask.hip, restated in numpy by
 * tests/verify_mask_stages.py).  The choice among candidates is cp_select_poses.
 * cp_verify_poses_mask: P poses (poses, cam_K, k_stride, verts .. Vmax as cp_render_depth) are rendered tile by tile over the masks'
 *   W x H frame -- no depth frame and no dense mask is stored -- and every model pixel (render D > 0) is tested against its mask's bit.
 *   full_bits int32 (NM,H,WW), WW = ceil(W / 32), with full_area int32 (NM): the full (amodal) masks as cp_coco_pack / cp_paste_masks
 *   leave them (pixel x = bit x & 31 of word x >> 5); vis_bits / vis_area: the visible masks in the same layout, both or both NULL;
 *   mask_ids int32 (P) or NULL (then NM == P and pose p reads mask p); status int32 (P) or NULL: a pose whose entry is 0 is not a candidate.
 *   Outputs: counts int32 (P,5) = n_model (D > 0) n_inter (model and full) n_vis_in (model and visible; 0 without) n_mask
 *   (full_area[m], read) n_vis (vis_area[m], read; 0 without); box int32 (P,4) = xmin ymin xmax ymax of the model pixels, -1s when
 *   n_model == 0; iou = n_inter / (n_model + n_mask - n_inter), cover = n_vis_in / n_vis, score = iou, all fp64 (P); ok uint8 (P).
 *   score and iou are NaN with ok = 0 when the union is 0 or the pose is not counted (its three sums 0, its box -1s): a non-finite pose
 *   or cam_K, a vertex at Z <= 0, a mesh id out of range, a mask id outside 0..NM-1 (n_mask = n_vis = 0 then), status 0.  cover is NaN
 *   when n_vis == 0, without the visible masks, or when the pose is not counted.  labels uint8 (P,H,W) or NULL: model | full << 1 |
 *   visible << 2 per pixel; a pose that is not counted still gets its mask bits.  scratch: cp_verify_poses_mask_scratch_bytes(P, Vmax)
 *   bytes (0 = bad arguments), 16-byte aligned.  Four launches; every output is a function of integer sums: bitwise the same alone or
 *   in a batch, with or without labels.
 * CP_ERR_INVALID: a null pointer, the mesh / view argument rules of the raster family, NM <= 0, no mask_ids although NM != P, one of
 * vis_bits / vis_area without the other; CP_ERR_ALIGN; CP_ERR_RANGE: H * W > 2^24 (the sums are int32), too many blocks. */
size_t cp_verify_poses_mask_scratch_bytes(int P, int Vmax);
int cp_verify_poses_mask(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                         const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                         const int32_t* full_bits, const int32_t* full_area, const int32_t* vis_bits, const int32_t* vis_area,
                         const int32_t* mask_ids, int NM, int H, int W, const int32_t* status, int P, int Vmax, int32_t* counts,
                         int32_t* box, double* score, double* iou, double* cover, uint8_t* ok, uint8_t* labels, void* scratch);

/* The poses of an image verified together against the visible masks (row N31): row N28 with occlusion between the estimates.  The
 * reference does not verify; opt-in, the rule is this project's own (stated in full at the top of csrc/scene_verify_mask.hip, restated
 * in numpy by tests/scene_verify_stages.py).  The choice among candidates is cp_select_poses.
 * cp_verify_scene_mask: P poses (poses, cam_K, k_stride, verts .. Vmax as cp_render_depth; cam_K per POSE with k_stride 9) are rendered
 *   tile by tile, depth only, over the masks' W x H frame; pose p belongs to image image_ids[p] (0 .. I-1), int32 (P) on the device.
 *   Its slot is its rank among the poses of its image in the order given (-1 for an image id out of range); at most 32 poses per image
 *   take part.  The counted poses of an image give the composite ren = the smallest positive depth (cp_render_scene's), and a model pixel
 *   (D > 0) of pose p is PREDICTED VISIBLE where cp_render_scene's 'bop19' test holds with ren as the sensor depth: f32(dist_p) -
 *   f32(dist_ren) <= f32(delta), both distances under pose p's cam_K.  full_bits / full_area, vis_bits / vis_area: the full and the
 *   visible masks as in cp_verify_poses_mask, BOTH required; mask_ids int32 (P) or NULL (then NM == P); status int32 (P) or NULL.
 *   A pose is not counted -- it occludes nothing, its sums are 0, its boxes -1s, ok = 0, its quotients NaN -- with a non-finite pose or
 *   cam_K, a vertex at Z <= 0, a mesh, mask or image id out of range, status 0, or a slot >= 32.
 *   Outputs: counts int32 (P,8) = n_model n_pvis (predicted visible) n_inter (model and full) n_vis_in (model and visible) n_pvis_in
 *   (pvis and visible) n_mask (full_area[m], read) n_vis (vis_area[m], read) n_hidden_seen (n_vis_in - n_pvis_in); boxes int32 (P,2,4) =
 *   xmin ymin xmax ymax of the model pixels and of the predicted-visible pixels, -1s without any; slot int32 (P); fp64 (P): iou =
 *   n_inter / (n_model + n_mask - n_inter) and cover = n_vis_in / n_vis (cp_verify_poses_mask's bits and NaNs), iou_vis = n_pvis_in /
 *   (n_pvis + n_vis - n_pvis_in), visib_fract = n_pvis / n_model (NaN when n_model == 0), score = iou_vis; ok uint8 (P): 0 with
 *   iou_vis = score = NaN when that union is 0 or the pose is not counted.  plane_full, plane_visib int32 (I,H,W), both or both NULL:
 *   bit s is set where the pose at slot s has a model / a predicted-visible pixel (cp_render_scene's planes).  scratch:
 *   cp_verify_scene_mask_scratch_bytes(P, Vmax, I) bytes (0 = bad arguments), 16-byte aligned.  Five launches; every output is a
 *   function of integer sums and per-pixel values: bitwise the same for an image alone or in a batch, with or without the planes.
 * CP_ERR_INVALID: a null pointer, the mesh / view argument rules of the raster family, NM <= 0, no mask_ids although NM != P, I <= 0,
 * one plane without the other, a delta that is negative, not finite or no float32; CP_ERR_ALIGN; CP_ERR_RANGE: H * W > 2^24 (the sums
 * are int32), too many blocks. */
size_t cp_verify_scene_mask_scratch_bytes(int P, int Vmax, int I);
int cp_verify_scene_mask(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                         const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                         const int32_t* full_bits, const int32_t* full_area, const int32_t* vis_bits, const int32_t* vis_area,
                         const int32_t* mask_ids, int NM, int H, int W, const int32_t* image_ids, int I, const int32_t* status,
                         double delta, int P, int Vmax, int32_t* counts, int32_t* boxes, int32_t* slot, double* score, double* iou,
                         double* cover, double* iou_vis, double* visib_fract, uint8_t* ok, int32_t* plane_full, int32_t* plane_visib,
                         void* scratch);

/* Hypothesis verification of poses against the photograph (row N35): the colour term beside rows N26 / N28 / N31, which see geometry
 * only.  The reference does not verify; opt-in, RGB-only, the rule is this project's own (stated in full at the top of
 * csrc/pose_verify_photo.hip, restated in numpy by tests/photo_stages.py).  The choice among candidates is cp_select_poses.
 * cp_verify_poses_photo: P poses (poses, cam_K, k_stride, verts .. mesh_ids, colors, normals, surf_color, light_pos, ambient_weight,
 *   shading as cp_render_rgb) are rendered and shaded tile by tile over the frames' W x H grid -- cp_render_rgb's colour and depth bits
 *   at ssaa 1; no frame, render or dense mask is stored -- and correlated with frame image_ids[p] (int32 (P) or NULL: then I == 1) of
 *   frames uint8 (I,H,W,3), RGB, or B G R with bgr != 0.  Luma Y = (77 R + 150 G + 29 B + 128) >> 8 of both; the pixel set is D > 0,
 *   intersected with bit (y, x) of visible mask row mask_ids[p] when vis_bits int32 (NM,H,WW), WW = ceil(W / 32) (cp_coco_pack's /
 *   cp_paste_masks' layout) is given (mask_ids int32 (P) or NULL: then NM == P; without vis_bits NM == 0 and mask_ids NULL).
 *   status int32 (P) or NULL: a pose whose entry is 0 is not a candidate.  min_pixels >= 2, no default.
 *   Outputs: counts int32 (P,2) = n_model (D > 0) n (the pixel set); sums int64 (P,5) = Sa Sb Saa Sbb Sab (a: the render's luma, b: the
 *   frame's); fp64 (P): with cov = n Sab - Sa Sb, va = n Saa - Sa^2, vb = n Sbb - Sb^2 exact in int64, ncc = cov / sqrt(va * vb),
 *   score = ncc, gain = cov / va, offset = (Sb - gain Sa) / n; ok uint8 (P): 0 with the four NaN when va == 0, vb == 0, n < min_pixels
 *   or the pose is not counted (zero sums): a non-finite pose or cam_K, a singular R, a vertex at Z <= 0, a mesh, image or mask id out
 *   of range, status 0.  scratch: cp_verify_poses_photo_scratch_bytes(P, Vmax) bytes (0 = bad arguments), 16-byte aligned.  Four
 *   launches; integer atomics only; every output is a function of integer sums: bitwise the same alone or in a batch.
 * cp_verify_poses_photo_tex: the same plus cp_render_rgb_tex's five texture arguments (all NULL: the plain call).
 * CP_ERR_INVALID: a null pointer, the mesh / view / image / shading / texture argument rules of cp_render_rgb_tex, min_pixels < 2,
 * NM <= 0 with masks, no mask_ids although NM != P, NM or mask_ids without masks; CP_ERR_ALIGN; CP_ERR_RANGE: H * W > 2^22 (a tile's
 * sums are int32, a pose's products int64), too many blocks. */
size_t cp_verify_poses_photo_scratch_bytes(int P, int Vmax);
int cp_verify_poses_photo(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                          const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                          const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                          double ambient_weight, int shading, const uint8_t* frames, const int32_t* image_ids, int I, int H, int W,
                          int bgr, const int32_t* vis_bits, const int32_t* mask_ids, int NM, const int32_t* status, int min_pixels,
                          int P, int Vmax, int32_t* counts, int64_t* sums, double* ncc, double* score, double* gain, double* offset,
                          uint8_t* ok, void* scratch);
int cp_verify_poses_photo_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                              const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                              const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                              double ambient_weight, int shading, const uint8_t* frames, const int32_t* image_ids, int I, int H, int W,
                              int bgr, const int32_t* vis_bits, const int32_t* mask_ids, int NM, const int32_t* status, int min_pixels,
                              int P, int Vmax, int32_t* counts, int64_t* sums, double* ncc, double* score, double* gain,
                              double* offset, uint8_t* ok, void* scratch, const float* uv, const uint32_t* texels,
                              const int32_t* tex_off, const int32_t* tex_dims, int filter);

/* Silhouette refinement of poses against predicted masks (row N30): row N24 for RGB-only data.  The reference does not refine; opt-in,
 * the rule is this project's own (stated in full at the top of csrc/mask_refine.hip, restated in numpy by tests/mask_refine_stages.py).
 * cp_mask_extents: bits int32 (NM,H,WW), WW = ceil(W / 32), as cp_coco_pack / cp_paste_masks leave them -> row int32 (NM,H,2) = (first,
 *   last) set column of every row, col int32 (NM,W,2) = (first, last) set row of every column, (-1, -1) where there is none; bits at
 *   columns >= W are ignored.  One launch, integer only, no atomics.
 * cp_contour_samples (stage A): one raster pass of P poses (poses, cam_K, k_stride, verts .. Vmax, H, W as cp_render_depth), then per
 *   pose the first / last covered pixel of at most grid lattice rows and the topmost / bottommost of at most grid lattice columns (row
 *   N24's lattice, grid in 1..64); S = 4 grid slots: 2 j (+ 1) for lattice row j, 2 grid + 2 i (+ 1) for lattice column i.
 *   Outputs: rect int32 (P,4), shape int32 (P,2) as cp_surface_samples; pixel int32 (P,S,2) (-1 -1 = empty slot: no covered pixel on the
 *   line, or the pixel lies on the frame's border), depth fp32 (P,S) (cp_render_depth's bits at the pixel, 0 in an empty slot), X fp64
 *   (P,S,3) the sample's model-space point (NaN in an empty slot), ok int32 (P) (0: not rendered).  scratch:
 *   cp_contour_samples_scratch_bytes(P, Vmax, grid) bytes (0 = bad arguments), 16-byte aligned.  Four launches; 64-bit integer atomic
 *   min / max merge the extremes across tiles, nothing else.
 * cp_mask_refine (stages B and C): ONE launch, one workgroup per pose, fp64 without contraction.
 *   pose_in fp64 (P,12) = [R row-major | t]; cam_K fp64 with k_stride 0 or 9; X, pixel, ok, grid: cp_contour_samples' outputs for THESE
 *   poses; row, col: cp_mask_extents' outputs over NM masks of the H x W frame; mask_ids int32 (P) or NULL (then NM == P and pose p reads
 *   mask p; an id outside 0..NM-1 passes the pose through); max_dist fp64 (P), pixels; status_in int32 (P) or NULL: 0 = leave this pose
 *   alone; dof 0 = translation only (R is returned bitwise), 1 = rotation and translation; max_iters in 1..64; step_tol > 0, finite;
 *   min_pairs >= 6.
 *   Outputs: pose_out, status_out, info (cp_mask_refine_info_doubles() = 42), records (cp_mask_refine_record_doubles() = 18 per
 *   iteration, or NULL) as cp_icp_refine's.
 * CP_ERR_INVALID: a null pointer, the mesh / view argument rules of the raster family, NM <= 0, no mask_ids although NM != P, a grid,
 * dof, max_iters, step_tol or min_pairs outside its range, a partial overlap of the poses; CP_ERR_ALIGN; CP_ERR_RANGE: H * W >= 2^31,
 * too many blocks. */
int cp_mask_extents(cp_stream_t stream, const int32_t* bits, int NM, int H, int W, int32_t* row, int32_t* col);
size_t cp_contour_samples_scratch_bytes(int P, int Vmax, int grid);
int cp_contour_samples(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                       const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                       int H, int W, int P, int Vmax, int grid, int32_t* rect, int32_t* shape, int32_t* pixel, float* depth,
                       double* X, int32_t* ok, void* scratch);
int cp_mask_refine_record_doubles(void);
int cp_mask_refine_info_doubles(void);
int cp_mask_refine(cp_stream_t stream, const double* pose_in, const double* cam_K, int k_stride, const double* X, const int32_t* pixel,
                   const int32_t* ok, int grid, const int32_t* row, const int32_t* col, const int32_t* mask_ids, int NM, int H, int W,
                   const double* max_dist, const int32_t* status_in, int dof, int max_iters, double step_tol, int min_pairs, int P,
                   double* pose_out, int32_t* status_out, double* info, double* records);

/* Rotation / translation errors, symmetry-aware (row N23): bop_toolkit_lib.pose_error.re / .te (pose_error.py:187-214) for P pose
 * pairs, the rotation error optionally against the closest symmetric copy of the second pose (checkerpose/test_lm.py:33-55,
 * get_closest_rot).  The rule is stated in full at the top of csrc/rete.hip and restated in numpy by tests/rete_stages.py.  One
 * launch, one wave per pair, fp64 without contraction, no atomics.
 *   pose_a, pose_b fp64 (P,12) = [R row-major | t] (P == 0 returns without a launch);
 *   syms fp64 (sumS,12) + s_offsets int32 (M+1) on the device (cp_bop_errors' layout; only the rotation part of a row is read) with
 *   s_offsets_host, the same M + 1 words in host memory, checked before anything is launched: [0] == 0 and ascending (an empty set
 *   is allowed); mesh_ids int32 (P) on the device, or NULL with M == 1; mesh_ids_host: the same P words in host memory, or NULL
 *   (then an id outside [0, M) is met on the device: that pair gets re = cos = NaN, index -1).  syms == NULL: no symmetries, the
 *   plain re / te (its four companions must be NULL too, M is not read).
 * Candidates in order: index -1 is R_b itself, then R_b . S_k, k = 0 .. S-1; cos_k = 1 + 0.5 sum((R_a - R_cand) o cof R_cand) /
 * det R_cand; re_k = degrees(acos(clamp(cos_k, -1, 1))), NaN where cos_k is not finite; the winner is the FIRST candidate with the
 * smallest re_k (strict <, NaN never replaces, a NaN plain candidate stays).  te = |t_b - t_a|.
 * Outputs: re fp64 (P) in degrees, te fp64 (P), cos fp64 (P) or NULL (the winner's cos_k before the clamp), index int32 (P) or NULL.
 * CP_ERR_INVALID: a null pointer, P < 0, M < 1, offsets that do not start at 0 or do not ascend, a host mesh id outside [0, M),
 * companions of a table that is not given.  CP_ERR_ALIGN: a pointer not aligned to its element. */
int cp_pose_rete(cp_stream_t stream, const double* pose_a, const double* pose_b, int P, const double* syms, const int32_t* s_offsets,
                 const int32_t* s_offsets_host, int M, const int32_t* mesh_ids, const int32_t* mesh_ids_host, double* re, double* te,
                 double* cos_out, int32_t* index);
/* The pass counts of the reference's LM report (test_lm.py:306-327) per object slot: counts int32 (n_obj, cp_rete_pass_columns() = 10)
 * = [n, adx < 0.02 d, adx < 0.05 d, adx < 0.1 d, re < 2 & te < 20, re < 5 & te < 50, re < 2, re < 5, te < 20, te < 50], every `<`
 * strict, a NaN error counted as 10000 first.  re, te, adx, diam fp64 (P), slot int32 (P) on the device; slot_host: the same P words
 * in host memory, or NULL (then a slot outside [0, n_obj) is skipped on the device).  counts is zeroed first (one hipMemsetAsync),
 * then one launch: LDS partial sums per workgroup, integer atomics after them -- the result does not depend on the order.
 * CP_ERR_INVALID: a null pointer, P < 0, n_obj outside 1..256, a host slot outside [0, n_obj). */
int cp_rete_pass_columns(void);
int cp_rete_pass_counts(cp_stream_t stream, const double* re, const double* te, const double* adx, const double* diam,
                        const int32_t* slot, const int32_t* slot_host, int P, int n_obj, int32_t* counts);

/* Pose errors on the device (next-row N5; reference metric.py:8-18 -> bop_toolkit_lib/pose_error.py:147-184, called once per image
 * by test.py:378-427 / test_lm.py:300-321): ADD = mean_i |P_est(p_i) - P_gt(p_i)| and ADD-S / ADI = mean_i min_j |P_gt(p_i) - P_est(p_j)|
 * over an object's mesh vertices, for B poses at once.
 *   pose_est, pose_gt fp64 (B,12) = [R row-major | t], the layout cp_pnp_ransac writes;
 *   verts fp32 (sumV,3): the vertices of M meshes packed one after the other (16-byte aligned base), offsets int32 (M+1) with mesh m
 *   at rows [offsets[m], offsets[m+1]); mesh_id int32 (B) names each pose's mesh (NULL = mesh 0 for all).  offsets NULL = ONE mesh
 *   of Vmax vertices (M is ignored; mesh_id must be NULL too).  Vmax >= the largest mesh a pose refers to.
 *   kinds: CP_POSE_ERR_ADD | CP_POSE_ERR_ADI, at least one; add / adi fp64 (B) are written for the kinds asked (the other may be NULL).
 * Arithmetic: the relative pose Rr = I + R_est^T (R_gt - R_est) (= R_est^T R_gt for an orthonormal R_est, exactly I for equal poses),
 * tr = R_est^T (t_gt - t_est) in fp64, then fp32 in the model frame: q_i = Rr p_i + tr, ADD = mean |q_i - p_i|, ADI = mean min_j
 * |q_i - p_j| with direct-difference distances (no |q|^2 + |p|^2 - 2 q.p expansion), one square root per query, means summed in
 * fp64 in a fixed order that depends on the mesh alone: results are bit-identical from call to call and do not depend on B.
 * Error against the fp64 definition: a few fp32 roundings of (largest vertex norm + |tr| + error).  ADI costs V^2 distance
 * evaluations per pose (all pairs, no spatial index).  A pose whose mesh id lies outside [0, M) or whose mesh is empty or larger
 * than Vmax, or whose relative pose is not finite, gets NaN in both errors.  CP_ERR_RANGE: more than 2^24 - 1 workgroups (about
 * B * ceil(Vmax / 1024) of them) -- split the batch.  scratch: cp_pose_errors_scratch_bytes(B, Vmax) bytes, 16-byte aligned (needed for ADI only). */
enum { CP_POSE_ERR_ADD = 1, CP_POSE_ERR_ADI = 2 };
size_t cp_pose_errors_scratch_bytes(int B, int Vmax);
int cp_pose_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const float* verts, const int32_t* offsets,
                   int M, const int32_t* mesh_id, int B, int Vmax, int kinds, double* add, double* adi, void* scratch);

/* BOP's MSSD, MSPD and projection error on the device (next-row N7; csrc/bop_error.hip; reference bop_toolkit_lib/pose_error.py:96-144
 * mssd / mspd, :217-232 proj -- the errors eval_bop19_pose.py scores the LM-O / YCB-V tables by), for B poses at once.  With
 * R_gs = R_gt R_s, t_gs = R_gt t_s + t_gt over the symmetry transformations s of the pose's mesh:
 *   MSSD = min_s max_v |R_est p_v + t_est - (R_gs p_v + t_gs)|,   MSPD = min_s max_v |proj_est(p_v) - proj_gs(p_v)|  (pixels),
 *   proj = mean_v |proj_est(p_v) - proj_gt(p_v)| (no symmetries),  proj_X(p) = first two rows of K [R | t] p_h over the third
 *   (misc.project_pts: no guard on the depth; a vertex at depth exactly 0 is outside the contract).
 *   pose_est, pose_gt fp64 (B,12) = [R row-major | t] as cp_pose_errors; cam_K fp64 row-major 3x3: (B,9) with k_stride = 9 or ONE
 *   matrix with k_stride = 0;  verts fp32 (sumV,3) + v_offsets int32 (M+1): cp_pose_errors' vertex table (v_offsets NULL = one mesh
 *   of Vmax vertices, M == 1);  syms fp64 (sumS,12) = [R_s row-major | t_s] + s_offsets int32 (M+1): mesh m owns the symmetry rows
 *   [s_offsets[m], s_offsets[m+1]) (at least one: the identity is NOT implied);  mesh_ids int32 (B), or NULL when M == 1.
 *   Vmax / Smax >= the largest mesh / symmetry set a pose refers to.
 *   kinds: CP_BOP_ERR_MSSD | _MSPD | _PROJ, at least one; mssd / mspd / proj fp64 (B) are written for the kinds asked (the others
 *   may be NULL).  Optionally CP_BOP_MAP_SMALL or CP_BOP_MAP_LARGE forces one of the two mappings of the main pass (measurement
 *   and tests: the results are bit-identical either way; scratch then comes from cp_bop_errors_map_scratch_bytes with that bit).
 * Arithmetic: everything per (pose, symmetry) -- R_gs, t_gs, D_s = R_est - R_gs, d_s = t_est - t_gs, K [R_est | t_est],
 * K [R_gs | t_gs] -- is formed once in fp64 without contraction and rounded to fp32; the loop over the vertices is fp32:
 * MSSD as |D_s p + d_s|^2 (linear in the difference: the translations never cancel in the loop), the estimate's projection once
 * per vertex, maxima over SQUARED distances, one fp64 square root per (pose, symmetry), proj's distances summed in fp64 in a
 * fixed order.  Every output is bit-identical from call to call, for a pose alone or in a batch, whichever kinds are asked and
 * whichever mapping runs.  A pose with a non-finite entry in either pose or in its K, a mesh id outside [0, M), a mesh that is
 * empty or larger than Vmax or a symmetry set that is empty or larger than Smax scores NaN in every kind asked.
 * At most three launches (compose, main pass, final reduction), nothing allocates or synchronises.  CP_ERR_RANGE: a launch of
 * 2^24 workgroups or more -- split the batch.  scratch: cp_bop_errors_scratch_bytes(B, Smax, Vmax) bytes, 16-byte aligned. */
enum { CP_BOP_ERR_MSSD = 1, CP_BOP_ERR_MSPD = 2, CP_BOP_ERR_PROJ = 4, CP_BOP_MAP_SMALL = 16, CP_BOP_MAP_LARGE = 32 };
size_t cp_bop_errors_scratch_bytes(int B, int Smax, int Vmax);
size_t cp_bop_errors_map_scratch_bytes(int B, int Smax, int Vmax, unsigned map);   /* map: 0 (as the call chooses), CP_BOP_MAP_SMALL or _LARGE */
int cp_bop_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                  const float* verts, const int32_t* v_offsets, const double* syms, const int32_t* s_offsets, int M,
                  const int32_t* mesh_ids, int B, int Vmax, int Smax, unsigned kinds, double* mssd, double* mspd, double* proj,
                  void* scratch);

/* BOP's Visible Surface Discrepancy on the device (next-row N8; csrc/vsd_error.hip; reference bop_toolkit_lib/pose_error.py:17-93 vsd,
 * misc.py:110-163 depth_im_to_dist_im_fast, visibility.py in 'bop19' mode, the 'step' cost): a depth rasteriser fused with the
 * reference's pixel counting, for B poses at once.
 * Render rule (renderer_py.py:185-226, 422-555): depth[y, x] is the smallest eye-space Z > 0 at which the ray through image point
 * (x + 0.5, y + 0.5) meets a triangle of the mesh under K' [R | t], K' = (fx, fy, cx, cy) of cam_K with skew 0; Z is the triangle
 * plane's (perspective-correct); no back-face culling; background 0; triangles of zero area are skipped.
 *   pose_est, pose_gt, cam_K, k_stride, verts, v_offsets, mesh_ids: as cp_bop_errors (v_offsets is required);
 *   faces int32 (sumF,3) + f_offsets int32 (M+1): mesh m owns the rows [f_offsets[m], f_offsets[m+1]), vertex indices LOCAL to the
 *   mesh (a triangle with an index outside [0, V_m) is skipped);
 *   depth_test fp32 (I,H,W) in the vertices' units (mm), image_ids int32 (B) names each pose's image (NULL when I == 1);
 *   delta: the visibility tolerance (compared in fp32, as the reference's fp32 difference is); diameters fp64 (M), device;
 *   taus: T <= 16 doubles ON THE HOST (copied into the launch); normalized_by_diameter: |dist_gt - dist_est| / diameter first;
 *   sphere_check != 0: the caller's shortcut of eval_calc_errors.py:299-318 -- when misc.overlapping_sphere_projections(diameter / 2,
 *   t_est, t_gt) is false the pose is not rendered and every error is 1.0 (counts 0).
 * Writes errors fp64 (B,T) = (count(dists >= tau) + union - inter) / union (1.0 when union == 0) and counts int32 (B,T+2) =
 * union, inter, count per tau.  depth_out fp32 (B,2,H,W) (estimate, ground truth), or NULL: the counts do not depend on it.
 * A pose with a non-finite entry (either pose or K), a mesh id outside [0, M), an image id outside [0, I), a mesh that is empty or
 * larger than Vmax, or ANY vertex at Z <= 0 in either pose scores NaN in every tau (counts 0).
 * The distance arithmetic is the reference's in fp64 (integer pixel x, y -- not the sample point); every output is a function of
 * integer pixel counts: bit-identical from call to call, for a pose alone or in a batch, with or without depth_out.  Four launches
 * (pose, vertex, tile, sum), nothing allocates or synchronises.  CP_ERR_RANGE: 2^24 workgroups or more (B * ceil(W/32) * ceil(H/32)
 * tiles) -- split the batch.  scratch: cp_vsd_errors_scratch_bytes(B, Vmax, H, W) bytes, 16-byte aligned.
 * cp_vsd_from_depth: the same counting on caller-supplied depth images depth_est, depth_gt fp32 (B,H,W); diameters fp64 (B), one
 * per pose; scratch: cp_vsd_errors_scratch_bytes(B, 0, H, W).  Three launches (pose, tile, sum).
 * cp_render_depth: poses + meshes -> depth_out fp32 (B,H,W) alone (a pose that is not rendered gives zeros); three launches;
 * scratch as cp_vsd_errors. */
size_t cp_vsd_errors_scratch_bytes(int B, int Vmax, int H, int W);
int cp_vsd_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                  const float* verts, const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                  const int32_t* mesh_ids, const float* depth_test, const int32_t* image_ids, int I, int H, int W,
                  double delta, const double* diameters, const double* taus, int T, int normalized_by_diameter,
                  int sphere_check, int B, int Vmax, double* errors, int32_t* counts, float* depth_out, void* scratch);
int cp_vsd_from_depth(cp_stream_t stream, const float* depth_est, const float* depth_gt, const double* cam_K, int k_stride,
                      const float* depth_test, const int32_t* image_ids, int I, int H, int W, double delta,
                      const double* diameters, const double* taus, int T, int normalized_by_diameter, int B, double* errors,
                      int32_t* counts, void* scratch);
int cp_render_depth(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                    const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                    int H, int W, int B, int Vmax, float* depth_out, void* scratch);

/* BOP ground-truth info and masks on the device (next-row N10; csrc/gt_info.hip; reference bop_toolkit scripts/calc_gt_info.py:72-175
 * and scripts/calc_gt_masks.py:94-127): what scene_gt_info.json, mask/ and mask_visib/ hold, for B ground-truth poses at once.
 * The object is rendered (cp_vsd_errors' render rule and rasteriser, csrc/vsd_raster.h) on the frame's pixel grid EXTENDED to
 * x in [-W, 2W), y in [-H, 2H) -- the reference's 3W x 3H canvas with the principal point moved by (W, H), in frame coordinates.
 * The canvas's 32 x 32 tile grid starts at (-32 ceil(W/32), -32 ceil(H/32)): frame pixel (0, 0) is a tile corner, and the in-frame
 * depth is bit-identical to cp_render_depth's at (H, W).
 *   poses fp64 (B,12) [R row-major | t]; cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, Vmax: as cp_render_depth;
 *   depth fp32 (I,H,W), the sensor's depth in the vertices' units (mm; 0 = no measurement), image_ids int32 (B) (NULL when I == 1);
 *   delta: the visibility tolerance, compared in fp32 as in cp_vsd_errors.
 * With dist_gt / dist_im = depth_im_to_dist_im_fast of the in-frame render / of depth (fp64, integer pixel x, y):
 *   mask = dist_gt > 0;  mask_visib = (f32(dist_gt) - f32(dist_im) <= delta or dist_im == 0) and dist_gt > 0   ('bop19')
 *   counts int32 (B,3) = px_count_all (canvas pixels with depth > 0), px_count_valid (mask pixels with dist_im > 0), px_count_visib;
 *   visib_fract fp64 (B) = visib / (double)all, 0.0 when all == 0;
 *   boxes int32 (B,2,4) = bbox_obj (the canvas silhouette, frame coordinates, not clipped), bbox_visib (of mask_visib): each
 *   [xmin, ymin, xmax - xmin, ymax - ymin]; BOTH are -1 -1 -1 -1 unless px_count_visib > 0;
 *   ok uint8 (B): 0 for a pose that is not rendered -- a non-finite entry (pose or K), a mesh id outside [0, M), an image id outside
 *   [0, I), a mesh that is empty or larger than Vmax, or ANY vertex at Z <= 0: counts 0, visib_fract 0, boxes -1, images 0;
 *   mask, mask_visib uint8 (B,H,W) holding 0 / 255 (both or neither; NULL to skip), depth_gt fp32 (B,H,W) the in-frame render (or NULL).
 * Tiles outside the pose's vertex rectangle leave at once, the canvas margin does no distance arithmetic, no image is stored unless
 * asked.  Integer reductions only (wave shuffles, LDS, order-independent integer atomics): every output is bit-identical from call
 * to call, for a pose alone or in a batch, with or without the optional images.  Four launches (pose, vertex, tile, finish), nothing
 * allocates or synchronises.  CP_ERR_RANGE: 2^24 workgroups or more (B * 9 ceil(W/32) ceil(H/32) tiles at most) -- split the batch.
 * scratch: cp_gt_info_scratch_bytes(B, Vmax) bytes, 16-byte aligned.
 * cp_gt_info_from_depth: the same counting on a caller-supplied canvas depth_gt_large fp32 (B,3H,3W) (frame pixel (x, y) is
 * [y + H][x + W]); three launches (pose, tile, finish); scratch: cp_gt_info_scratch_bytes(B, 0). */
size_t cp_gt_info_scratch_bytes(int B, int Vmax);
int cp_gt_info(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
               const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
               const float* depth, const int32_t* image_ids, int I, int H, int W, double delta, int B, int Vmax, int32_t* counts,
               double* visib_fract, int32_t* boxes, uint8_t* ok, uint8_t* mask, uint8_t* mask_visib, float* depth_gt, void* scratch);
int cp_gt_info_from_depth(cp_stream_t stream, const float* depth_gt_large, const double* cam_K, int k_stride, const float* depth,
                          const int32_t* image_ids, int I, int H, int W, double delta, int B, int32_t* counts, double* visib_fract,
                          int32_t* boxes, uint8_t* ok, uint8_t* mask, uint8_t* mask_visib, void* scratch);

/* Shaded RGB training frames of coloured meshes on the device (next-row N14; csrc/render_rgb.hip; reference bop_toolkit
 * scripts/render_train_imgs.py:128-214 with renderer_py.py:24-105, 422-518 in mode 'rgb'): uint8 frames of B poses at once.
 * Coverage and the front-most surface are cp_render_depth's rule and arithmetic (csrc/vsd_raster.h); among triangles of equal 1 / Z
 * the smallest face index wins.  Over the winning triangle v_color, v_L = normalize(light - eye_pos) per VERTEX and v_normal are
 * interpolated perspective-correctly;  light_w = min(1, ambient_weight + max(dot(normalize(v_L), normalize(n)), 0));
 * rgb = round-half-even(255 * light_w * v_color) on the fp32 value, clamped to 0..255; elsewhere the quantised bg_color.
 *   shading 0 (flat): n = the unit face normal turned towards the viewer whatever the winding (the shader's cross(dFdx, dFdy));
 *   shading 1 (phong): n = the interpolated v_normal = normalize(u_nm * vec4(a_normal, 1)).xyz, u_nm = inverse([R t; 0 1])^T -- the
 *   shader's FOUR-vector normalisation, kept: the per-vertex lengths differ and weight the interpolation.  Needs normals.
 *   poses, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, Vmax: as cp_render_depth;
 *   colors fp32 (sumV,3) in [0, 1], rows as verts, or NULL: every vertex has surf_color; normals fp32 (sumV,3) or NULL (flat);
 *   surf_color, light_pos, bg_color: 3 doubles each ON THE HOST; light_pos in the camera frame of the poses (x right, y down,
 *   z forward: the reference's light_cam_pos with y and z negated);
 *   ssaa 1, 2 or 4: samples on the ssaa-times finer grid under K * ssaa, each quantised to uint8, then ssaa x ssaa samples averaged
 *   as integers: (s + 2) >> 2, or round-half-even of s / 16 -- equal bit for bit to a plain render at (ssaa W, ssaa H) under
 *   K * ssaa averaged so (the project's statement of cv2.INTER_AREA on 8-bit images, not pinned against cv2);
 *   bgr != 0: the channels are stored in reverse order.
 * Writes rgb uint8 (B,H,W,3) and ok uint8 (B): 0 for a pose that is not rendered (a non-finite entry of the pose or K, a singular R,
 * a mesh id outside [0, M), a mesh that is empty or larger than Vmax, ANY vertex at Z <= 0): background only, depth and mask 0,
 * box -1.  Optional, ssaa == 1 only (NULL to skip; CP_ERR_INVALID with ssaa > 1): depth fp32 (B,H,W), bit-identical to
 * cp_render_depth's; mask uint8 (B,H,W) = 255 where depth > 0; boxes int32 (B,4) = xmin, ymin, xmax - xmin, ymax - ymin of the
 * mask (misc.calc_2d_bbox), -1 -1 -1 -1 when it is empty.
 * Four launches (pose, vertex, tile, finish) whatever the data and the options; a workgroup per (pose, 32 x 32 tile of the sample
 * grid); tiles outside the pose's vertex rectangle store the background and leave.  Integer reductions only (LDS integer sums of
 * the samples, wave shuffles and one order-independent integer atomic per box limit and tile): every output is bit-identical from
 * call to call, for a pose alone or in a batch, with or without the optional outputs.  Nothing allocates or synchronises.
 * CP_ERR_RANGE: 2^24 workgroups or more (B * ceil(ssaa W / 32) * ceil(ssaa H / 32) tiles) -- split the batch.
 * Scratch layout: B headers of 48 4-byte words [P 12 | rect 4 | bad | ok | R t 12 | normal matrix 12 | box 4 | sign | spare],
 * rounded up to 16 bytes, then four float4 (B, Vmax) tables (screen record, eye position, v_L, v_normal), each rounded up to 16
 * bytes.  cp_render_rgb_scratch_bytes(B, Vmax) bytes, 16-byte aligned. */
size_t cp_render_rgb_scratch_bytes(int B, int Vmax);
int cp_render_rgb(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                  const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                  const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                  double ambient_weight, const double* bg_color, int shading, int ssaa, int bgr, int H, int W, int B, int Vmax,
                  uint8_t* rgb, float* depth, uint8_t* mask, int32_t* boxes, uint8_t* ok, void* scratch);

/* Textured meshes (next-row N20; csrc/render_shade.h states the rule; reference bop_toolkit_lib/renderer_py.py:309-352 add_object and the
 * fragment shaders' texture2D(u_texture, v_texcoord), the sampler pinned to the OpenGL specification's NEAREST / LINEAR rule with
 * CLAMP_TO_EDGE and no mipmaps -- which filter vispy selects, a driver's fixed-point filtering and OpenGL's output are NOT pinned).
 * cp_render_rgb_tex, cp_vis_poses_tex and cp_render_scene_tex take their plain call's arguments plus five:
 *   uv fp32 (sumV,2) = (texture_u, texture_v), rows as verts (zeros for a mesh without a texture);
 *   texels uint32 (sum Wt Ht): one word r | g << 8 | b << 16 per texel, every texture row-major in the image FILE's row order (row 0 on
 *   top; GL's texel row j is the file's row Ht - 1 - j: the flip is in the index), textures in mesh order;
 *   tex_off int32 (M+1): each mesh's first texel;  tex_dims int32 (M,2) = Wt, Ht, both in 1..16384, or 0 0: the mesh has no texture;
 *   filter 0 (nearest) or 1 (linear).
 * Per covered sample of a textured mesh (u, v) is interpolated perspective-correctly with v_color's weights and expression form;
 *   nearest: i = clamp(floor(u Wt), 0, Wt - 1), j = clamp(floor(v Ht), 0, Ht - 1), texel = T[Ht - 1 - j][i];
 *   linear:  a = u Wt - 0.5, i0 = floor(a), alpha = a - i0, i1 = i0 + 1, both clamped; likewise j0, j1, beta; per channel in fp32 on the
 *            bytes  lo = t00 + alpha (t10 - t00), hi = t01 + alpha (t11 - t01), texel = lo + beta (hi - lo);
 *   colour = light_w * (texel / 255) (a correctly rounded fp32 division), quantised as every other colour.
 * Priority: a surface colour (cp_vis_poses / cp_render_scene: surf_colors non-NULL) ignores the texture; else a textured mesh uses its
 * texture and its vertex colours are ignored; else the vertex colours; else the surface colour / 0.5 grey.  (cp_render_rgb_tex's
 * surf_color is never NULL: it colours the untextured meshes when colors is NULL; a caller who wants it to override passes no tables.)
 * The four tables are given together or all NULL (CP_ERR_INVALID otherwise, and for an unknown filter); all NULL is the plain call,
 * bit for bit and launch for launch -- the plain entry points forward so.  With tables the tile launch is the tile kernel's textured
 * instantiation (rgb_tile_kernel<true>, vis_scene_tile_kernel<true>, scene_tile_kernel<true>: same launch count, same scratch).  The tables are trusted as verts and v_offsets are: the caller checks them (scene.MeshSet does). */
int cp_render_rgb_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                      const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                      const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                      double ambient_weight, const double* bg_color, int shading, int ssaa, int bgr, int H, int W, int B, int Vmax,
                      uint8_t* rgb, float* depth, uint8_t* mask, int32_t* boxes, uint8_t* ok, void* scratch, const float* uv,
                      const uint32_t* texels, const int32_t* tex_off, const int32_t* tex_dims, int filter);
int cp_vis_poses_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                     const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                     const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                     const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host, const int32_t* pose_order_host,
                     const uint8_t* frames, int shading, double ambient_weight, const double* light_pos, const double* box_color,
                     int resolve, int draw_boxes, int H, int W, int P, int I, int Vmax, uint8_t* vis, uint8_t* ren_rgb, float* ren_depth,
                     int32_t* boxes, uint8_t* ok, void* scratch, const float* uv, const uint32_t* texels, const int32_t* tex_off,
                     const int32_t* tex_dims, int filter);
int cp_render_scene_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                        const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                        const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                        const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host, const int32_t* pose_order_host,
                        const uint8_t* backgrounds, int n_bg, const int32_t* bg_index, const double* bg_color, int shading,
                        double ambient_weight, const double* light_pos, double delta, int bgr, int H, int W, int P, int I, int Vmax,
                        uint8_t* rgb, float* depth, uint32_t* full_bits, uint32_t* visib_bits, int32_t* slot, int32_t* counts,
                        double* visib_fract, int32_t* boxes, uint8_t* ok, void* scratch, const float* uv, const uint32_t* texels,
                        const int32_t* tex_off, const int32_t* tex_dims, int filter);

/* Poses drawn over the photograph on the device (next-row N18; csrc/vis_poses.hip; reference bop_toolkit_lib/visualization.py:90-235
 * vis_object_poses as scripts/vis_est_poses.py and vis_gt_poses.py drive it, text excluded): for I images and P poses at once,
 * the composite of every image's poses, their 2-D boxes, and the half-and-half blend with the frame.
 * Per image, poses in the order given: m_rgb / m_depth of a pose are cp_render_rgb's (ssaa 1, background 0 0 0) of that pose alone, bit
 * for bit, with the pose's row of surf_colors fp64 (P,3) (NULL: the mesh's colours, 0.5 grey without any);  ren_rgb = 0, ren_depth = 0;
 *   m = m_depth != 0 and (ren_depth == 0 or m_depth < ren_depth) on the fp32 depths (strict: the earlier of two equal depths stays);
 *   ren_depth[m] = m_depth;  resolve 1: ren_rgb[m] = m_rgb;  resolve 0: ren_rgb = min(255, ren_rgb + m_rgb) as integers;
 *   boxes int32 (P,4) = x, y, xmax - xmin, ymax - ymin over the pixels where ANY channel of m_rgb is > 0 (a black surface occludes
 *   but has no box), -1 four times without any;  with draw_boxes 1 a pixel on the one-pixel outline through (x, y), (x + w, y + h) of
 *   any box of its image adds int(c * 255) of box_color (3 doubles ON THE HOST, as light_pos: cp_render_rgb's);
 *   vis uint8 (I,H,W,3) = min(255, (frames + ren_rgb) / 2 + outline) as integers;  ren_rgb uint8 (I,H,W,3), ren_depth fp32 (I,H,W).
 *   ok uint8 (P): 0 for a pose that is not rendered (cp_render_rgb's rule, an image id outside [0, I), a non-finite surface colour):
 *   it is skipped, its box is -1.
 * cam_K fp64 (9) shared (k_stride 0) or (I,9) PER IMAGE (k_stride 9); image_of_pose int32 (P); the CSR img_off int32 (I+1) /
 * pose_order int32 (P) -- the poses of image i in drawing order -- on the device AND, the same values, in host memory
 * (img_off_host, pose_order_host: checked before anything is launched -- img_off[0] == 0, monotone, img_off[I] == P, every entry of
 * pose_order in [0, P): CP_ERR_INVALID otherwise).  The other mesh arguments, shading, ambient_weight: as cp_render_rgb.
 * Four launches whatever the data (pose, vertex, scene tile: a workgroup per (image, 32 x 32 tile) that keeps the per-pose frames in
 * registers, finish: per pixel); integer reductions only; every output is bit-identical from call to call, for an image alone or in
 * a batch.  Nothing allocates or synchronises.  CP_ERR_RANGE: 2^24 workgroups or more in a launch, or I * H * W * 3 >= 2^31.
 * scratch: cp_vis_poses_scratch_bytes(P, Vmax, I) bytes (cp_render_rgb's layout for P poses), 16-byte aligned.
 * cp_depth_diff_vis (visualization.py:206-235, depth_for_vis :76-88): for I renders ren_depth fp32 (I,H,W) against sensor depths depth
 * fp32 (n_depth,H,W), image_ids int32 (I) naming each render's (NULL: image i when n_depth == I, image 0 when n_depth == 1):
 *   valid = depth > 0 and ren_depth > 0;  dd = valid ? ren_depth - depth : 0 (fp32);  red = 255 where valid and dd < (float)delta;
 *   m0 = min dd over ALL pixels;  x = dd - m0 (fp32);  over x > 0, in fp64: n = (x - mn) / (mx / s) + 0.2 with mn = min x,
 *   mx = max (x - mn), s = the caller's 1.0 - 0.2;  green = blue = (uint8)(255 n);  everything 0 where not valid.
 *   out uint8 (I,H,W,3);  stats fp64 (I,3) = min, max, mean of dd over the valid pixels (NaN without any; the mean is a fixed-order
 *   fp64 sum);  diff_ok uint8 (I): 0 when dd holds fewer than three distinct values (the reference raises or divides 0 by 0): zeros.
 * Five launches; minima and maxima through order-preserving integer keys and integer atomics, no floating-point atomics.
 * scratch: cp_depth_diff_vis_scratch_bytes(I, H, W) bytes, 16-byte aligned. */
size_t cp_vis_poses_scratch_bytes(int P, int Vmax, int I);
int cp_vis_poses(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                 const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                 const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                 const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host, const int32_t* pose_order_host,
                 const uint8_t* frames, int shading, double ambient_weight, const double* light_pos, const double* box_color,
                 int resolve, int draw_boxes, int H, int W, int P, int I, int Vmax, uint8_t* vis, uint8_t* ren_rgb, float* ren_depth,
                 int32_t* boxes, uint8_t* ok, void* scratch);
size_t cp_depth_diff_vis_scratch_bytes(int I, int H, int W);
int cp_depth_diff_vis(cp_stream_t stream, const float* ren_depth, const float* depth, const int32_t* image_ids, int n_depth,
                      double delta, double s, int H, int W, int I, uint8_t* out, double* stats, uint8_t* diff_ok, void* scratch);

/* Occluded multi-object training scenes with their labels on the device (next-row N19; csrc/scene_labels.hip): for I images and P poses
 * at once, the composite colour and depth of every image over a background, and for every pose the content of scene_gt_info.json
 * with that composite as the sensor depth, the 2 P mask images held as two bit planes per image.  Inputs follow cp_vis_poses (poses,
 * per-IMAGE cam_K / k_stride, the mesh tables, colors, normals, surf_colors, image_of_pose, the img_off / pose_order CSR on the device
 * and on the host); there are no frames.
 * Slots.  The slot s of a pose is its rank among the poses of its image, in the order given (pose_order within [img_off[i],
 *   img_off[i + 1])).  Poses that are not rendered keep their slot.  At most 32 poses per image (CP_ERR_RANGE otherwise).
 * Composite.  depth fp32 (I,H,W) and the colour are exactly what cp_vis_poses produces with resolve != 0: per pose cp_render_rgb's frame
 *   (ssaa 1); the front-most pose wins under the strict m_depth < ren_depth test: of equal depths the earlier pose keeps the pixel.
 *   rgb uint8 (I,H,W,3) = the winner's colour where depth > 0; elsewhere backgrounds[bg_index[img]] (backgrounds uint8 (n_bg,H,W,3),
 *   bg_index int32 (I); bg_index NULL: row img when n_bg == I, row 0 when n_bg == 1; a row outside [0, n_bg) falls back to bg_color), or,
 *   with backgrounds NULL (then n_bg == 0 and bg_index NULL), the quantised bg_color (3 doubles ON THE HOST, cp_render_rgb's rounding).
 *   bgr != 0 stores every pixel's channels reversed.
 * Labels.  Exactly cp_gt_info's for every pose with the image's composite depth as the sensor depth: the same canvas x in [-W, 2W),
 *   y in [-H, 2H) on the same tile origin, the same depth_im_to_dist_im_fast arithmetic, the same 'bop19' test
 *   f32(dist_gt) - f32(dist_im) <= (float)delta.  counts int32 (P,3) = px_count_all, _valid, _visib; visib_fract fp64 (P); boxes int32
 *   (P,2,4) = bbox_obj, bbox_visib as x, y, w, h, BOTH -1 unless px_count_visib > 0; ok uint8 (P).
 *   A pose that cp_vis_poses does not render (a non-finite entry, a singular R, any vertex at Z <= 0, a bad mesh or image id, a
 *   non-finite surface colour) has ok = 0, counts 0, fraction 0, boxes -1 and no bit.
 * Bit planes.  full_bits and visib_bits uint32 (I,H,W): bit s of a pixel is set where the mask / mask_visib image of the pose at slot s
 *   of that image would be 255: 8 bytes per pixel whatever P is.  slot int32 (P): each pose's slot (-1: its image id is out of range).
 * Four launches whatever the data (pose, vertex, tile: a workgroup per (image, 32 x 32 canvas tile) -- margin tiles count coverage only,
 * in-frame tiles make the composite depth in a first walk over the image's poses and the labels, bits and the owner's colour in a
 * second --, finish).  Integer reductions only, no floating-point atomics; nothing allocates or synchronises; every output is
 * bit-identical from call to call, for an image alone or in a batch, with or without backgrounds (the labels).
 * CP_ERR_RANGE: more than 32 poses in an image, 2^24 workgroups or more in a launch, I * H * W * 3 or n_bg * H * W * 3 >= 2^31.
 * scratch: cp_render_scene_scratch_bytes(P, Vmax, I) bytes -- P headers of 64 4-byte words, then cp_render_rgb's four float4 tables of
 * (P, Vmax) --, 16-byte aligned. */
size_t cp_render_scene_scratch_bytes(int P, int Vmax, int I);
int cp_render_scene(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                    const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                    const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                    const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host, const int32_t* pose_order_host,
                    const uint8_t* backgrounds, int n_bg, const int32_t* bg_index, const double* bg_color, int shading,
                    double ambient_weight, const double* light_pos, double delta, int bgr, int H, int W, int P, int I, int Vmax,
                    uint8_t* rgb, float* depth, uint32_t* full_bits, uint32_t* visib_bits, int32_t* slot, int32_t* counts,
                    double* visib_fract, int32_t* boxes, uint8_t* ok, void* scratch);

/* BOP's overlap errors on the device (next-row N12; csrc/mask_error.hip; reference bop_toolkit_lib/pose_error.py:235-330 cou_mask, cus,
 * cou_bb, cou_bb_proj with misc.calc_2d_bbox / misc.iou, misc.py:202-263): the four functions that close pose_error.py.
 * cp_mask_errors: for B pairs (estimate, ground truth) of one mesh each under one K, on a W x H frame,
 *   cus fp64 (B) = 1 - inter / (double)union of the two silhouettes, 1.0 when union == 0;
 *   cou_bb_proj fp64 (B) = 1 - misc.iou of the silhouettes' boxes (xmin, ymin, xmax - xmin, ymax - ymin): no + 1, not clipped, the
 *   intersection counted only when its width AND height are > 0.  Where a side's silhouette is EMPTY the reference raises (xs.min() of
 *   nothing): NaN here.  (Either output may be NULL, not both.)
 * A pixel of a side is set exactly where cp_render_depth's depth at (H, W) is > 0 (the render rule and rasteriser of cp_vsd_errors,
 * csrc/vsd_raster.h).  pose_est, pose_gt, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, Vmax: as cp_vsd_errors.
 * A pair with a non-finite entry (either pose, K), a mesh id outside [0, M), a mesh that is empty or larger than Vmax, or ANY vertex
 * at Z <= 0 on either side is not scored: ok = 0, both errors NaN, counts 0, boxes -1, masks 0.
 * sphere_check != 0 (needs diameters fp64 (M)): misc.overlapping_sphere_projections(diameter / 2, t_est, t_gt) decided on the device,
 * as eval_calc_errors.py:299-302,357-362 applies it to 'cus' ALONE: where it fails cus = 1.0 and -- unless cou_bb_proj is asked, which
 * the shortcut never touches -- the pair is not rendered (counts 0, boxes -1, masks 0).  The launch list does not depend on it.
 * Optional outputs (NULL to skip): counts int32 (B,4) = inter, union, n_est, n_gt; boxes int32 (B,2,4) = the estimate's and the
 * ground truth's x, y, w, h (-1 -1 -1 -1 for an empty silhouette); ok uint8 (B); masks uint8 (B,2,H,W) holding 0 / 1.
 * With masks asked no tile leaves early: every tile of every pair stores its pixels (zeros where nothing is rendered).
 * Scratch layout: B headers of 52 4-byte words [P_est 12 | P_gt 12 | rect_est 4 | rect_gt 4 | bad 2 | ok | skip | render | inter
 * union n_est n_gt | est xmin ymin xmax ymax | gt xmin ymin xmax ymax | 3 spare], rounded up to 16 bytes, then the screen records
 * float4 (B, 2, Vmax).  cp_mask_errors_scratch_bytes(B, Vmax) bytes, 16-byte aligned.
 * Four launches (pose, vertex, tile, finish); a workgroup per (pair, 32 x 32 tile) rasterises BOTH sides, so intersection and union
 * are decided in registers; tiles outside both vertex rectangles leave at once.  Integer reductions only (wave shuffles, LDS, one
 * order-independent integer atomic per value and tile): every output is bit-identical from call to call, for a pair alone or in a
 * batch, with or without the optional outputs.  Nothing allocates or synchronises.  CP_ERR_RANGE: 2^24 workgroups or more.
 * cp_mask_overlap: the counting half on caller-supplied masks uint8 (B,H,W), nonzero = set (any alignment): the same counts and boxes,
 * cou_mask fp64 (B) (pose_error.cou_mask) and cou_bb fp64 (B) of the masks' boxes (NaN where a mask is empty); each output may be
 * NULL, not all.  ONE launch, a workgroup per pair, no scratch.
 * cp_box_overlap: out fp64 (B) = 1 - misc.iou(bb_est, bb_gt) (pose_error.cou_bb) of B box pairs x, y, w, h given as fp64 (B,4), in fp64
 * without contraction in the reference's order of operations.  One launch. */
size_t cp_mask_errors_scratch_bytes(int B, int Vmax);
int cp_mask_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                   const float* verts, const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                   const int32_t* mesh_ids, const double* diameters, int H, int W, int sphere_check, int B, int Vmax, double* cus,
                   double* cou_bb_proj, int32_t* counts, int32_t* boxes, uint8_t* ok, uint8_t* masks, void* scratch);
int cp_mask_overlap(cp_stream_t stream, const uint8_t* mask_est, const uint8_t* mask_gt, int H, int W, int B, double* cou_mask,
                    double* cou_bb, int32_t* counts, int32_t* boxes);
int cp_box_overlap(cp_stream_t stream, const double* bb_est, const double* bb_gt, int B, double* out);

/* BOP's matching of estimates to ground truths and its recall scores on the device (next-row N11; csrc/bop_match.hip; reference
 * bop_toolkit_lib/pose_matching.py:9-90 match_poses and score.py:62-137 calc_localization_scores), for every (scene, image, object)
 * group and every threshold column at once.
 * cp_bop_match.  Group g owns the estimates [est_off[g], est_off[g+1]) of est_score fp64 (NE) / est_ids int32 (NE) -- in the order of
 * the reference's `errs` list -- and the ground-truth slots [gt_off[g], gt_off[g+1]) in increasing gt_id; slot s writes output row
 * gt_rows[s] (int32 (NG), a permutation; NULL = the slot itself).  Its errors are the n_e x n_g rows of errs fp64 (P, C_err) starting
 * at row pair_off[g] (int64 (G+1)), estimate-major.  gt_valid uint8 (NG), by OUTPUT ROW (NULL = all valid).  Column c compares the
 * error columns col_err int32 (C, E) against the thresholds col_th fp64 (C, E), E = 1 or 2.  max_ests > 0: only the first max_ests
 * estimates in score order are matched (match_poses' max_ests_count).
 * Semantics, exactly match_poses': estimates by decreasing score, ties in list order (a NaN score sorts last); for each, the valid
 * and still unmatched ground truths are scanned in slot order and a candidate replaces the best so far only if EVERY element is
 * STRICTLY below it, the best so far starting at the thresholds; NaN and inf never match.
 * Outputs per (row, column): out_est int32 (NG, C) the matched estimate's est_ids entry or -1; out_score fp64 (NG, C); out_err and
 * out_norm = error / threshold (fp64 division) fp64 (NG, C, E); an unmatched entry holds -1.0 (the reference's defaults).
 * A group whose ground truths number more than 64 (or every group, with CP_BOP_MATCH_SCRATCH_MASK) keeps its matched set in
 * ceil(n_g / 64) words of scratch starting at word mask_off[g] (int32 (G); mask_words = their total; a group whose words are missing
 * or out of range stays unmatched, as does one whose table entries point outside NE / P).  CP_BOP_MATCH_NO_LDS reads the errors
 * where they lie instead of staging a group's block (<= 4096 doubles) through LDS.  The flags change no output bit.
 * One launch, a workgroup per group, a lane per column; nothing allocates or synchronises; bit-identical from call to call, for a
 * group alone or in a batch, a column alone or among others.  scratch: cp_bop_match_scratch_bytes(NE, mask_words, C), 16-byte aligned.
 * cp_bop_scores.  est_ids = cp_bop_match's out_est (NG, C); gt_obj / gt_scene int32 (NG): each row's index into the caller's object /
 * scene list (a row with an index outside [0, n_obj) / [0, n_scene) counts nowhere); groups as above.  counts int32 (NB, 1 + C) laid
 * out as [NB target counts | NB x C true positives], NB = 1 + n_obj + n_scene, bin 0 = total, 1 + o = object o, 1 + n_obj + s =
 * scene s: targets of a group = min(n_top, its valid ground truths), or their number when n_top <= 0; true positives = valid rows
 * with est_id != -1.  Integer reductions only (LDS bins when NB <= 128 and CP_BOP_SCORES_NO_LDS is not set, integer atomics).
 * Three launches (zero, targets, tp).  The quotients tp / (double)targets and their means are the caller's. */
#define CP_BOP_MATCH_NO_LDS 1u
#define CP_BOP_MATCH_SCRATCH_MASK 2u
#define CP_BOP_SCORES_NO_LDS 1u
size_t cp_bop_match_scratch_bytes(int NE, long long mask_words, int C);
int cp_bop_match(cp_stream_t stream, const double* errs, long long P, int C_err, const double* est_score, const int32_t* est_ids,
                 int NE, const int32_t* est_off, const int32_t* gt_off, const long long* pair_off, int G, const int32_t* gt_rows,
                 const uint8_t* gt_valid, int NG, const int32_t* col_err, const double* col_th, int C, int E, int max_ests,
                 const int32_t* mask_off, long long mask_words, unsigned flags, int32_t* out_est, double* out_score,
                 double* out_err, double* out_norm, void* scratch);
int cp_bop_scores(cp_stream_t stream, const int32_t* est_ids, const uint8_t* gt_valid, const int32_t* gt_obj,
                  const int32_t* gt_scene, int NG, const int32_t* gt_off, const int32_t* gt_rows, int G, int C, int n_obj,
                  int n_scene, int n_top, unsigned flags, int32_t* counts);

/* Ground-truth side on the device (next-row N6; csrc/targets.hip).
 *
 * cp_encode_targets: the labels of the reference's data loader (bop_dataset_pytorch.py:293,356-380: project the N keypoints through
 * K [R|t], discretise against the crop's FINAL box, MSB-first codes; lm_dataset_pytorch.py:393,438-462 with a per-sample object) for B
 * crops in one launch.
 *   p3d fp64, original units: (N,3) shared (p3d_bstride 0), (B,N,3) (p3d_bstride 3 N), or -- with obj_ids int32 (B), 1-based, device --
 *   the object table (n_obj,N,3); cam_K fp64 3x3 row-major (K_bstride 0 shared | 9); R fp64 (B,9) row-major, t fp64 (B,3);
 *   boxes int32 (B,4) x, y, w, h on the device = get_final_Bbox's result, S = crop_size_gt, a power of two in 8 .. 256 (bits = log2 S).
 *   boxes_host: the same (B,4) values in HOST memory, no_detection_host: uint8 (B) in host memory or NULL -- read before the launch:
 *   a flagged crop must carry the loader's dummy box (w = h = 0, :328-338) and gets all-zero labels; any other box needs w > 0 and
 *   h > 0 (CP_ERR_INVALID otherwise, nothing is launched).
 * Outputs (device): roi_mask_bit f32 (B,1,N); pixel_x_code, pixel_y_code f32 (B,bits,N) in {0,1}, MSB first; x_id, y_id int32 (B,N),
 * the ids after the clip to [0, S-1]; optional (NULL to skip) proj_xy fp64 (B,N,2) and depth fp64 (B,N).
 * Arithmetic: fp64 in the reference's order, compiled without floating-point contraction; u = x / z, id = trunc((u - bx) / (bw / S)),
 * out of the RoI = u < bx or v < by or id >= S.  The conversion saturates at the int32 range (numpy's astype(int) is undefined there);
 * a NaN quotient is out of the RoI with id 0. */
int cp_encode_targets(cp_stream_t stream, const double* p3d, long long p3d_bstride, const int32_t* obj_ids, int n_obj,
                      const double* cam_K, long long K_bstride, const double* R, const double* t, const int32_t* boxes,
                      const int32_t* boxes_host, const uint8_t* no_detection_host, int B, int N, int S, float* roi_mask_bit,
                      float* pixel_x_code, float* pixel_y_code, int32_t* x_id, int32_t* y_id, double* proj_xy, double* depth);

/* cp_code_report: the code / mask figures test.py prints beside ADD (:432-457), one workgroup per crop.
 *   pred_roi f32 (B,1,N), pred_x / pred_y f32 (B,nb,N) LOGITS (rows N apart, `*_bstride` elements between crops: slices of the
 *   network's logit block work as they are), nb <= bits (a truncated `stage`); seg f32 (B,2,H,W) logits [visible | full];
 *   gt_roi (B,1,N), gt_x / gt_y (B,bits,N): cp_encode_targets' labels, the first nb code rows are compared;
 *   mask_visib / mask_full (B,S,S): uint8 (non-zero = set) or, with mask_f32 = 1, f32 (> 0.5 = set), read at the positions
 *   F.interpolate(mode="nearest") takes for an (H,W) output (test.py:320-323).  Decisions are logit > 0.
 * counts int32 (B, 10 + 2 nb): n_in_roi, roi-bit mismatches, sum |x id difference| and sum |y id difference| inside the RoI (ids of
 *   the nb leading bits), visible mask: mismatching pixels, intersection, union, full mask: the same three, then the nb per-bit x
 *   mismatches and the nb per-bit y mismatches inside the RoI.
 * figures fp64 (B, 8 + 2 nb), formed from the counts as test.py does (npoint_in_roi clipped to >= 1; IoU = 1 for an empty union):
 *   roi_bit_acc, reproj_x_acc, reproj_y_acc, visib_pixel_acc, visib_iou, full_pixel_acc, full_iou, bit_err_arr[0 .. 2 nb].
 * Integer sums only (wave reductions + LDS, no atomics): bit-identical from call to call, independent of B. */
int cp_code_report(cp_stream_t stream, const float* pred_roi, long long roi_bstride, const float* pred_x, long long x_bstride,
                   const float* pred_y, long long y_bstride, int nb, const float* seg, int H, int W, const float* gt_roi,
                   const float* gt_x, const float* gt_y, int bits, const void* mask_visib, const void* mask_full, int mask_f32, int S,
                   int B, int N, int32_t* counts, double* figures);

/* Object preparation on the device (next-row N9; csrc/prepare.hip): the keypoints and the diameter every other row starts from.
 * Both entry points take M point clouds as one fp64 table pts (sumV,3) (8-byte aligned) + offsets int32 (M+1) on the device, cloud m
 * at rows [offsets[m], offsets[m+1]) -- MeshSet's layout in fp64 -- and offsets_host, the same M+1 values in HOST memory, read before
 * anything is launched: offsets_host[0] == 0 and every cloud holds at least one point (CP_ERR_INVALID otherwise).  M <= 65535.
 * All arithmetic is fp64 without contraction, square roots correctly rounded: results are numpy's bit for bit, identical from call
 * to call and for a cloud alone or in a batch.  Coordinates must be finite (the caller checks).  Nothing allocates or synchronises.
 *
 * cp_fps: farthest-point sampling by the reference's rule (preprocess_data/get_fps_points.py:65-90).  Start = (max + min) / 2 of the
 *   bounding box (not a vertex); every dist starts at (1.0 * sqrt((dx*dx + dy*dy) + dz*dz)) * 10 of the box extents; per sample
 *   d = sqrt((ex*ex + ey*ey) + ez*ez), e = p - farthest; if d < dist: dist = d; the next sample is the FIRST index of the largest dist
 *   (roots are compared, not squares).  npoint >= 1; npoint > V is legal (index 0 repeats once every dist is 0).
 *   ids int32 (M,npoint): indices local to each cloud; xyz fp64 (M,npoint,3): those points.
 *   slices: 0 = chosen from (M, largest cloud), or 1 .. 256 = the number of slices each cloud's dist is cut into (one workgroup
 *   each; tests and measurement: the output does not depend on it).  Launches: fps_bbox_kernel, then npoint + 1 of fps_step_kernel
 *   (cp_kernel_log lists the chain as ONE entry "fps_step_kernel x<npoint + 1>").
 *   scratch: cp_fps_scratch_bytes(M, sumV, Vmax, slices) bytes, 8-byte aligned (Vmax = the largest cloud; 0 = bad arguments).
 * cp_pts_diameter: diameters fp64 (M) = sqrt(max over all pairs of ((dx*dx + dy*dy) + dz*dz)) == bop_toolkit_lib.misc.calc_pts_diameter.
 *   V^2 / 2 pair evaluations per cloud in tiles of 1024 x 1024 (pts_diameter_kernel, then pts_diameter_finish_kernel).
 *   CP_ERR_RANGE: a cloud of more than 5792 * 1024 points.  scratch: cp_pts_diameter_scratch_bytes(M, Vmax) bytes, 8-byte aligned. */
size_t cp_fps_scratch_bytes(int M, long long sumV, int Vmax, int slices);
int cp_fps(cp_stream_t stream, const double* pts, const int32_t* offsets, const int32_t* offsets_host, int M, int npoint, int slices,
           int32_t* ids, double* xyz, void* scratch);
size_t cp_pts_diameter_scratch_bytes(int M, int Vmax);
int cp_pts_diameter(cp_stream_t stream, const double* pts, const int32_t* offsets, const int32_t* offsets_host, int M,
                    double* diameters, void* scratch);

/* Self-occlusion measure on the device (next-row N16; csrc/visibility.hip): the per-view rule of the reference's
 * preprocess_data/get_overall_visibility.py:20-42 (compute_vis_hpr: hidden point removal) for n_views poses of ONE cloud in one launch.
 * pts fp64 (V,3), R fp64 (n_views,3,3), t fp64 (3) with t_stride 0 or (n_views,3) with t_stride 3, all 8-byte aligned, on the device.
 * Per view: pc = R p + t, flipped = pc + 2 (radius - |pc|) pc / |pc| with radius = max |pc| * 10^radius_param, the convex hull of
 * the flipped points plus the viewpoint (0,0,0) by a bounded, deterministic insertion; a vertex is visible
 * when it is a vertex of that hull.  fp64 without contraction, no floating-point atomics; the outputs do not depend on the call,
 * on the batch a view is in, on the order of the views or on `workgroups`.
 *   counts int32 (V): the number of views with status 0 in which each vertex is visible (zeroed by the call).
 *   mask: null, or uint8 (n_views,V) of 0 / 1 (a view with nonzero status: zeros).
 *   status int32 (n_views): 0 ok; 1 degenerate cloud (the initial tetrahedron has a zero extent: coincident, collinear or coplanar
 *     flipped points); 2 a horizon that is not a simple cycle of at least 3 edges; 3 face table full; 4 more than V + 1 insertions;
 *     5 a vertex at the viewpoint (norm 0) or a non-finite norm / radius.  The caller reads it; a failing view never spins.
 *   workgroups: 0 = chosen from (n_views, V), or 1 .. 65535 = the number of workgroups that share the views (tests, measurement).
 *   scratch: cp_hpr_visibility_scratch_bytes(n_views, V, workgroups) bytes, 8-byte aligned (0 = bad arguments): one slab per
 *   WORKGROUP, not per view.  CP_ERR_INVALID: a null pointer (mask may be null), n_views < 1, V < 4, t_stride not 0 / 3,
 *   radius_param not in [0, 8] (NaN included), workgroups < 0; CP_ERR_RANGE: V > 2^22, workgroups > 65535.  One hipMemsetAsync and one
 *   launch (hpr_visibility_kernel); nothing allocates or synchronises. */
size_t cp_hpr_visibility_scratch_bytes(int n_views, int V, int workgroups);
int cp_hpr_visibility(cp_stream_t stream, const double* pts, const double* R, const double* t, int t_stride, int n_views, int V,
                      double radius_param, int workgroups, int32_t* counts, uint8_t* mask, int32_t* status, void* scratch);

/* ---------------------------------------------------------------------------------------------
 * Training side: backward of the fused graph ops + the loss head of train.py:307-320.
 * Gradients are fp32; `pq` is the forward's saved GEMM output in `dtype`.
 * ------------------------------------------------------------------------------------------- */

/* Backward of cp_edgeconv_gather_max == autograd of `x.max(dim=-1)` over get_graph_feature + LeakyReLU
 * (init.py:36-49,64-68): gq = gout * leaky'(max_k P' + Q');  dQ'[b,i] = gq;  dP'[b,j] = sum of gq over the edges
 * (i,k) with idx[i,k] == j that won the max (first arg-max).  gout (B,N,gout_cstride) fp32 (channels
 * [gout_coff, +C)), dpq (B,N,2C) fp32 fully overwritten.  rev_ptr (G,N+1) / rev_edge (G,N*K): the static graph's
 * reverse adjacency -- flat edge ids i*K+k stably sorted by idx[i,k] -- so the scatter is a deterministic gather.
 * workspace: cp_edgeconv_bwd_workspace_bytes(B,N,C) bytes. */
size_t cp_edgeconv_bwd_workspace_bytes(int B, int N, int C);
int cp_edgeconv_gather_max_bwd(cp_stream_t stream, int dtype, const void* pq, const int32_t* idx,
                               const int32_t* rev_ptr, const int32_t* rev_edge, const int32_t* graph_ids,
                               const float* gout, float* dpq, void* workspace, int B, int N, int K, int C,
                               int G, int gout_cstride, int gout_coff, float slope);

/* Backward of cp_index2feat_gather == autograd of the four advanced-index gathers + mask multiply
 * (pipeline.py:156-163,280): dpatches (B,Hp,Wp,E) fp32, zeroed then scatter-added (fp32 hardware atomics). */
int cp_index2feat_gather_bwd(cp_stream_t stream, const float* gout, const int32_t* x_id, const int32_t* y_id,
                             const float* mask, float* dpatches, int B, int N, int Hp, int Wp, int E, int k,
                             int gout_cstride, int gout_coff);
/* same with gout stored in `dtype` (the training program keeps activation gradients in the storage type) */
int cp_index2feat_gather_bwd_t(cp_stream_t stream, int dtype, const void* gout, const int32_t* x_id, const int32_t* y_id,
                               const float* mask, float* dpatches, int B, int N, int Hp, int Wp, int E, int k,
                               int gout_cstride, int gout_coff);

/* UnmaskedCodeLoss (mask == NULL; losses/code_loss.py:6-27) / MaskedCodeLoss (mask (B,N); code_loss.py:30-62):
 * pred (B,nbits,N) fp32 logits with batch stride pred_bstride (elements), gt likewise (train.py:312-313 passes the
 * slice pixel_x_codes[:, :num_proj_bits]).  loss_type CP_LOSS_BCE (BCEWithLogits) | CP_LOSS_L1 (L1 on sigmoid).
 * Writes loss[0] and, if dpred != NULL, d loss / d pred (same indexing, stride dpred_bstride).
 * workspace: cp_loss_workspace_bytes() bytes, 16-byte aligned. */
size_t cp_loss_workspace_bytes(void);
int cp_code_loss(cp_stream_t stream, int loss_type, const float* pred, long long pred_bstride, const float* gt,
                 long long gt_bstride, const float* mask, int B, int nbits, int N, float* loss, float* dpred,
                 long long dpred_bstride, void* workspace);

/* MaskedCodeLoss(loss_type="CE") (losses/code_loss.py:36-37,47-61; not used by train.py:87-88, kept for the class contract):
 * pred (B,C,N) fp32 class logits (batch stride pred_bstride), gt_class (B,N) class ids as fp32, mask (B,N):
 * loss = sum_bn mask * (logsumexp_c pred - pred[gt]) / clamp(sum mask, 1); dpred (optional) = d loss / d pred. */
int cp_masked_ce_loss(cp_stream_t stream, const float* pred, long long pred_bstride, const float* gt_class,
                      const float* mask, int B, int C, int N, float* loss, float* dpred, long long dpred_bstride,
                      void* workspace);

/* MaskLoss_interpolate (losses/mask_loss.py:6-17): mean | sigmoid(pred[b,0]) - nearest_resize(gt[b]) |.
 * pred points at channel 0 of the slice the caller passes (train.py:315-316: pred_seg[:, 0:1] / [:, 1:2]), (h,w)
 * contiguous with batch stride pred_bstride; gt (B,Hm,Wm) fp32 contiguous. */
int cp_mask_loss(cp_stream_t stream, const float* pred, long long pred_bstride, const float* gt, int B, int h,
                 int w, int Hm, int Wm, float* loss, float* dpred, long long dpred_bstride, void* workspace);

/* ---------------------------------------------------------------------------------------------
 * Training side, dense layers (reference train.py:319 `loss.backward()` through every
 * nn.Conv2d / nn.ConvTranspose2d / nn.Linear of the path).
 *
 * Weight gradient:  dw[dw_base + co*dw_sco + ci*dw_sci + r*dw_sr + s*dw_ss] +=
 *       sum_{b,oy,ox} dy[b,oy,ox,co] * x[b, oy*stride-pad+r, ox*stride-pad+s, ci]          (fp32 atomics)
 * dy (B,Ho,Wo,dy_cstride) and x (B,H,W,x_cstride) are channels-last `dtype` tensors (channel slices via *_coff);
 * the caller zeroes dw first.  nn.Conv2d weight (Cout,Cin,R,S): dw_sco = Cin*R*S, dw_sci = R*S, dw_sr = S, dw_ss = 1.
 * nn.ConvTranspose2d(k3,s2,p1,op1) weight (Cin_t,Cout_t,3,3): pass the layer INPUT as `dy` (coarse grid) and the
 * output gradient as `x` (fine grid), stride 2, pad 1 -- same strides.  Data-gradients need no entry point of their
 * own: they are cp_conv2d_igemm / cp_conv3x3_halo / cp_gemm_rows launches over dy with cp_weight_dgrad()'s weights.
 * ------------------------------------------------------------------------------------------- */
typedef struct CpWgradDesc {
  int32_t dtype;
  int32_t B, H, W;             /* x spatial size */
  int32_t Ho, Wo;              /* dy spatial size */
  int32_t Cout, dy_cstride, dy_coff;
  int32_t Cin, x_cstride, x_coff;
  int32_t R, S, stride, pad;
  int64_t dw_base, dw_sco, dw_sci, dw_sr, dw_ss;
} CpWgradDesc;
int cp_conv2d_wgrad(cp_stream_t stream, const CpWgradDesc* d, const void* dy, const void* x, float* dw);
/* same, with a caller-owned scratch buffer: the pixel-slice partial sums go through it (plain stores + one reduction
 * launch, deterministic) instead of through fp32 atomics -- measured ~30 G atomics/s made every launch cost >= 0.6 ms.
 * dw is still accumulated into (+=).  Any size works (it bounds the number of slices); 160 MiB never limits. */
int cp_conv2d_wgrad_ws(cp_stream_t stream, const CpWgradDesc* d, const void* dy, const void* x, float* dw, void* workspace,
                       size_t workspace_bytes);

/* Deferred reduction (training step: ~360 weight-gradient launches per backward, each followed by a latency-bound reduction of
 * its pixel-slice partials): cp_conv2d_wgrad_deferred launches ONLY the partial kernel into `workspace` (which must stay
 * untouched until the reduction ran: cp_conv2d_wgrad_scratch_bytes() bytes give the launcher its preferred slice count) and
 * fills *item on the HOST; cp_conv2d_wgrad_plan fills the same item without launching (static launch programs resolve it at
 * build time).  item->ws == NULL: the layer needs no reduction (atomics / direct stores).  cp_wgrad_reduce_batch runs any number
 * of owed reductions in ONE launch: items in DEVICE memory + the exclusive prefix sum (n + 1 entries) of
 * cp_wgrad_reduce_item_blocks() of each.  Sums in slice order: bit-identical to cp_conv2d_wgrad_ws. */
typedef struct CpWgradReduceItem {
  const float* ws; float* dw;
  int32_t S, GY, co_blocks, ci_blocks, R, Ssz, Cout, Cin, taps_in_block;
  long long dw_base, dw_sco, dw_sci, dw_sr, dw_ss;
} CpWgradReduceItem;
size_t cp_conv2d_wgrad_scratch_bytes(const CpWgradDesc* d);
int cp_conv2d_wgrad_deferred(cp_stream_t stream, const CpWgradDesc* d, const void* dy, const void* x, float* dw, void* workspace,
                             size_t workspace_bytes, CpWgradReduceItem* item);
int cp_conv2d_wgrad_plan(const CpWgradDesc* d, const void* dy, const void* x, float* dw, void* workspace, size_t workspace_bytes,
                         CpWgradReduceItem* item);
uint32_t cp_wgrad_reduce_item_blocks(const CpWgradReduceItem* item);
int cp_wgrad_reduce_batch(cp_stream_t stream, const CpWgradReduceItem* items_dev, const uint32_t* block_prefix_dev, int n_items,
                          uint32_t total_blocks);

/* Grouped weight gradients: the partial-sum launches of SEVERAL layers in one launch per kernel kind.  cp_conv2d_wgrad_item =
 * cp_conv2d_wgrad_plan that also describes the layer's partial-sum launch in `compute` (nothing is launched) and cuts the layer's
 * pixels for about `target_blocks` workgroups (0: a whole GPU's worth, as the single-layer launches do) -- a caller that groups
 * n layers hands each its share of ~512 workgroups, which shrinks the partial tiles by the same factor.  reduce->ws == NULL: the
 * layer adds with atomics, it owes no reduction.  cp_wgrad_group: `items_dev` = items of ONE kind in device memory, `prefix_dev`
 * the exclusive prefix sum (n_items + 1 entries) of item.blocks.  Results equal the single-layer launches' up to fp32 summation
 * order across slices. */
#define CP_WGRAD_ITEM_BYTES 160
enum { CP_WGRAD_ITEM_3X3 = 0, CP_WGRAD_ITEM_3X3_SMALL = 1, CP_WGRAD_ITEM_GENERIC_BF16 = 2, CP_WGRAD_ITEM_GENERIC_F32 = 3,
       CP_WGRAD_ITEM_3X3_S2_SMALL = 4 };      /* all-taps kernels: stride 1 (0, 1); stride 2, <= 32 x 32 channels (4) */
typedef struct CpWgradItem {
  int32_t kind;
  uint32_t blocks, gx, gy;
  unsigned long long params[CP_WGRAD_ITEM_BYTES / 8];      /* opaque: the kernel's parameter block */
} CpWgradItem;
int cp_conv2d_wgrad_item(const CpWgradDesc* d, const void* dy, const void* x, float* dw, void* workspace, size_t workspace_bytes,
                         int target_blocks, CpWgradItem* compute, CpWgradReduceItem* reduce);
int cp_wgrad_group(cp_stream_t stream, int kind, const CpWgradItem* items_dev, const uint32_t* prefix_dev, int n_items,
                   uint32_t total_blocks);

/* Optimizer step over ALL parameter tensors in one launch (the reference's train.py:244-246,320: optim.Adam(net.parameters(), lr) or
 * optim.SGD(..., momentum=0.9); optimizer.step() per batch).  items (device memory): parameter, its gradient and the optimizer state of
 * one tensor, fp32, n elements; prefix = exclusive prefix sum (n_items + 1) of cp_opt_item_blocks(n).  cp_adam_multi = torch.optim.Adam
 * (amsgrad off; weight_decay is L2, added to the gradient; `step` counts from 1 and must exceed every item's step0);
 * cp_sgd_multi = torch.optim.SGD (dampening 0, no nesterov; m = momentum buffer, first_step: buf := grad; momentum 0: m may be NULL). */
typedef struct CpOptItem {
  float* p; const float* g; float* m; float* v;
  uint64_t n;
  uint32_t step0, pad;       /* Adam: the tensor's own step count is `step` - step0 (torch counts per parameter) */
} CpOptItem;
uint32_t cp_opt_item_blocks(uint64_t numel);
int cp_adam_multi(cp_stream_t stream, const CpOptItem* items_dev, const uint32_t* prefix_dev, int n_items, uint32_t total_blocks, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step);
int cp_sgd_multi(cp_stream_t stream, const CpOptItem* items_dev, const uint32_t* prefix_dev, int n_items, uint32_t total_blocks, float lr,
                 float momentum, float weight_decay, int first_step);

/* Weights of the data-gradient of a stride-1 conv: w (Cout,Cin,R,S) fp32 -> wt (Cin,Cout,R,S) fp32 with both taps
 * flipped (wt[ci][co][r][s] = w[co][ci][R-1-r][S-1-s]); dx = conv(dy, wt, stride 1, pad R-1-pad).  (Stride-2 3x3
 * convs use the transposed=1 phase packing of cp_pack_conv_weight on w itself; ConvTranspose2d's data-gradient is a
 * plain stride-2 conv with w read as (Cout'=Cin_t, Cin'=Cout_t, 3, 3).) */
int cp_weight_dgrad(cp_stream_t stream, const float* w, int Cout, int Cin, int R, int S, float* wt);

/* Train-mode BatchNorm2d (nn.BatchNorm2d defaults: eps 1e-5, momentum 0.1; inside timm hrnet, init.py:60,
 * pipeline.py:51,189-208) over the M = B*H*W rows of a channels-last tensor, C logical channels.
 * cp_bn_train_stats: batch mean / biased variance (fp64 sums) -> scale = gamma*rstd, shift = beta - mean*scale (fp32
 * vectors of ceil16(C) entries, zero beyond C), mean / rstd saved for the backward; running_mean / running_var
 * updated in place with `momentum` (unbiased variance), NULL = skip.  gamma / beta NULL = 1 / 0.
 * workspace: cp_bn_workspace_bytes(C); one workspace may serve many layers on one stream. */
size_t cp_bn_workspace_bytes(int C);
int cp_bn_train_stats(cp_stream_t stream, int dtype, const void* x, int M, int C, int x_cstride, int x_coff,
                      const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                      float eps, float* scale, float* shift, float* mean, float* rstd, void* workspace);
/* y = act(x * scale[c] + shift[c] + res) elementwise (res optional; y may alias x or res). */
int cp_affine_act(cp_stream_t stream, int dtype, const void* x, int x_cstride, int x_coff, const float* scale,
                  const float* shift, const void* res, int res_cstride, int res_coff, void* y, int y_cstride, int y_coff,
                  int M, int C, int act, float slope);
/* Backward of y = act(BN(x) + res):  dz = dy * act'(y);  dres (+)= dz;  dgamma = sum dz*xhat;  dbeta = sum dz;
 * dx = gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)).  x == NULL selects the bias-only form (y = act(conv + b)):
 * dx = dz, dbeta = sum dz.  dx may alias dy.  workspace: cp_bn_bwd_workspace_bytes(C). */
size_t cp_bn_bwd_workspace_bytes(int C);
int cp_bn_train_bwd(cp_stream_t stream, int dtype, const void* dy, int dy_cstride, int dy_coff, const void* y,
                    int y_cstride, int y_coff, const void* x, int x_cstride, int x_coff, const float* mean,
                    const float* rstd, const float* gamma, int M, int C, int act, float slope, void* dx, int dx_cstride,
                    int dx_coff, void* dres, int dres_cstride, int dres_coff, int dres_accumulate, float* dgamma,
                    float* dbeta, void* workspace);

/* Two-launch forms of the same BatchNorm forward / backward (what the training program uses): the column sums go into a
 * caller-zeroed fp64 accumulator block of cp_bn_acc_doubles(C) doubles (8 replicated [sum | sum of squares] resp.
 * [sum dz | sum dz*xhat] pairs of ceil16(C) entries: block b adds into replica b % 8 to spread the atomic traffic) by hardware
 * fp64 atomics, and the consumer launch derives the per-channel coefficients in its prologue -- no finalize launch (670 of them
 * were 8.5 % of a training step).  cp_bn_apply also writes mean / rstd (C floats each) and updates the running statistics;
 * cp_bn_bwd_apply writes dgamma / dbeta.  One accumulator pair per layer and pass; zero them all with one cp_memset_zero. */
size_t cp_bn_acc_doubles(int C);
int cp_bn_stats_accumulate(cp_stream_t stream, int dtype, const void* x, int M, int C, int x_cstride, int x_coff, double* acc);
int cp_bn_apply(cp_stream_t stream, int dtype, const void* x, int x_cstride, int x_coff, const double* acc, const float* gamma,
                const float* beta, float* running_mean, float* running_var, float momentum, float eps, const void* res,
                int res_cstride, int res_coff, void* y, int y_cstride, int y_coff, int M, int C, int act, float slope,
                float* mean, float* rstd);
int cp_bn_bwd_accumulate(cp_stream_t stream, int dtype, const void* dy, int dy_cstride, int dy_coff, const void* y,
                         int y_cstride, int y_coff, const void* x, int x_cstride, int x_coff, const float* mean,
                         const float* rstd, int M, int C, int act, float slope, double* acc);
int cp_bn_bwd_apply(cp_stream_t stream, int dtype, const void* dy, int dy_cstride, int dy_coff, const void* y, int y_cstride,
                    int y_coff, const void* x, int x_cstride, int x_coff, const float* mean, const float* rstd,
                    const float* gamma, const double* acc, int M, int C, int act, float slope, void* dx, int dx_cstride,
                    int dx_coff, void* dres, int dres_cstride, int dres_coff, int dres_accumulate, float* dgamma, float* dbeta);

/* Grouped BatchNorm passes: the same pass (statistics / apply / backward sums / backward apply) of up to CP_BN_GROUP_MAX
 * INDEPENDENT layers in ONE launch -- the branches of an HRNet module at equal depth (timm HighResolutionModule.forward runs
 * them one after the other; at the reference's training batch of 32 each pass is a 5-13 us launch over 0.3-5 MB).
 * cp_bn_item_* take the arguments of cp_bn_stats_accumulate / cp_bn_apply / cp_bn_bwd_accumulate / cp_bn_bwd_apply, run the
 * same checks and fill one item on the HOST (nothing is launched).  cp_bn_group: `items_dev` = the items of ONE kind and
 * dtype copied to device memory, `prefix_dev` = exclusive prefix sum (n_items + 1 entries) of item.blocks, `lds_bytes` = the
 * largest item.lds_bytes.  Every item behaves exactly as its single-layer launch (same block plan, same arithmetic). */
#define CP_BN_ITEM_BYTES 192
#define CP_BN_GROUP_MAX 16
enum { CP_BN_ITEM_STATS = 0, CP_BN_ITEM_APPLY = 1, CP_BN_ITEM_BWD_SUMS = 2, CP_BN_ITEM_BWD_APPLY = 3 };
typedef struct CpBnItem {
  int32_t kind, dtype;
  uint32_t blocks, lds_bytes;
  unsigned long long params[CP_BN_ITEM_BYTES / 8];      /* opaque: the kernel's parameter block */
} CpBnItem;
int cp_bn_item_stats(int dtype, const void* x, int M, int C, int x_cstride, int x_coff, double* acc, CpBnItem* item);
int cp_bn_item_apply(int dtype, const void* x, int x_cstride, int x_coff, const double* acc, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, const void* res, int res_cstride,
                     int res_coff, void* y, int y_cstride, int y_coff, int M, int C, int act, float slope, float* mean, float* rstd,
                     CpBnItem* item);
int cp_bn_item_bwd_sums(int dtype, const void* dy, int dy_cstride, int dy_coff, const void* y, int y_cstride, int y_coff,
                        const void* x, int x_cstride, int x_coff, const float* mean, const float* rstd, int M, int C, int act,
                        float slope, double* acc, CpBnItem* item);
int cp_bn_item_bwd_apply(int dtype, const void* dy, int dy_cstride, int dy_coff, const void* y, int y_cstride, int y_coff,
                         const void* x, int x_cstride, int x_coff, const float* mean, const float* rstd, const float* gamma,
                         const double* acc, int M, int C, int act, float slope, void* dx, int dx_cstride, int dx_coff, void* dres,
                         int dres_cstride, int dres_coff, int dres_accumulate, float* dgamma, float* dbeta, CpBnItem* item);
int cp_bn_group(cp_stream_t stream, int dtype, int kind, const CpBnItem* items_dev, const uint32_t* prefix_dev, int n_items,
                uint32_t total_blocks, uint32_t lds_bytes);

/* Train-mode EdgeConv in factored form (StaticGraph_module init.py:54-68 with BatchNorm2d batch statistics over the
 * B*N*K edges), see csrc/train_edge.hip.  pq (B,N,2C) = raw node GEMM output [P | Q] (W rows [W1 ; W2-W1], no
 * affine); kstar (B,N,C) uint8 receives the arg-max neighbour slot; scale/shift/mean/rstd: C floats each.
 * Backward writes dpq (B,N,2C) `dtype` = [dP - dQ | dQ], the operand of the node GEMM's weight- and data-gradient
 * (cp_edge_weight_view mode 1), plus dgamma / dbeta.  rev_ptr (G,N+1), rev_edge (G,N*K): reverse adjacency as for
 * cp_edgeconv_gather_max_bwd.  workspace: cp_edge_train_workspace_bytes(B, C).  C % 16 == 0.  out / gout may be channel
 * slices of wider buffers: both calls refuse (CP_ERR_ALIGN) a slice that overruns its row (coff + C > cstride). */
size_t cp_edge_train_workspace_bytes(int B, int C);
int cp_edgeconv_train_fwd(cp_stream_t stream, int dtype, const void* pq, const int32_t* idx, const int32_t* graph_ids,
                          const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                          float eps, void* out, int out_cstride, int out_coff, uint8_t* kstar, float* scale, float* shift,
                          float* mean, float* rstd, void* workspace, int B, int N, int K, int C, int G, float slope);
int cp_edgeconv_train_bwd(cp_stream_t stream, int dtype, const void* pq, const int32_t* idx, const int32_t* rev_ptr,
                          const int32_t* rev_edge, const int32_t* graph_ids, const void* out, int out_cstride, int out_coff,
                          const uint8_t* kstar, const void* gout, int gout_cstride, int gout_coff, const float* gamma,
                          const float* mean, const float* rstd, void* dpq, float* dgamma, float* dbeta, void* workspace,
                          int B, int N, int K, int C, int G, float slope);
/* EdgeConv weight views: w (C', 2C) = [W1 | W2] -> mode 0: (2C', C) = [W1 ; W2 - W1] (forward node GEMM);
 * mode 1: (C, 2C') with out[c][c'] = W1[c'][c], out[c][C'+c'] = W2[c'][c] (data-gradient of the node GEMM over D). */
int cp_edge_weight_view(cp_stream_t stream, const float* w, int Cout, int Cin, int mode, float* out);

/* Backward of cp_upsample2x_bilinear_ac (gather form, deterministic; H == 1 / W == 1: the sum of both output rows / columns;
 * CP_ERR_INVALID for a negative out_coff / in_coff) and of ONE source of cp_fuse_sum_act
 * (dsrc (+)= sum over the 2^shift x 2^shift block of dout * [out > 0]). */
int cp_upsample2x_bilinear_ac_bwd(cp_stream_t stream, int dtype, const void* dout, void* din, int B, int H, int W, int C,
                                  int out_cstride, int out_coff, int in_cstride, int in_coff, int accumulate);
int cp_fuse_sum_act_bwd(cp_stream_t stream, int dtype, const void* dout, const void* out, void* dsrc, int B, int Hs, int Ws,
                        int C, int shift, int relu, int accumulate);
/* ... and every (output, term) pair of one fuse layer in ONE launch (the pairs write distinct gradient tensors): the item is
 * cp_fuse_sum_act_bwd's argument list checked and packed on the host, `blocks` its workgroup count; items_dev / prefix_dev as for
 * the other grouped launches (<= 64 items). */
typedef struct CpFuseBwdItem {
  const void* dout; const void* out; void* dsrc;
  int32_t Hs, Ws, CG, shift, relu, accumulate;
  uint64_t total;
} CpFuseBwdItem;
int cp_fuse_sum_act_bwd_item(int dtype, const void* dout, const void* out, void* dsrc, int B, int Hs, int Ws, int C, int shift, int relu,
                             int accumulate, CpFuseBwdItem* item, uint32_t* blocks);
int cp_fuse_sum_act_bwd_group(cp_stream_t stream, int dtype, const CpFuseBwdItem* items_dev, const uint32_t* prefix_dev, int n_items,
                              uint32_t total_blocks);
/* Backward of cp_maxpool3x3s2 (resnet34 stem): x (B,H,W,C) forward input, dout (B,H/2,W/2,C), din (+)= routed gradient
 * (first maximum of each window in row-major order takes it, as ATen's CPU kernel does). */
int cp_maxpool3x3s2_bwd(cp_stream_t stream, int dtype, const void* x, const void* dout, void* din, int B, int H, int W, int C,
                        int accumulate);

/* plumbing: stream-ordered zero fill / device copy (capturable), and a tensor (fp32 or `dtype`: src_dtype) with arbitrary element strides (the logit block,
 * NCHW seg logits, fp32 scatter targets) -> channels-last `dtype` (B, HW, Cphys) with zero padded channels. */
int cp_memset_zero(cp_stream_t stream, void* p, size_t nbytes);
int cp_strided_to_nhwc(cp_stream_t stream, int dtype, const void* src, int src_dtype, long long base, long long sb,
                       long long sp, long long sc, void* out, int B, int HW, int C, int Cphys);
int cp_memcpy_d2d(cp_stream_t stream, void* dst, const void* src, size_t nbytes);

/* ---------------------------------------------------------------------------------------------
 * Batched weight preparation (training): a step re-packs ~1100 live weight tensors; as individual ~4 us launches that
 * was a fifth of the step.  cp_pack_item_*() fill one CpPackItem each on the HOST (same arguments and the same packed
 * image as the single-launch entry points they mirror), the caller keeps the items in DEVICE memory together with an
 * exclusive prefix sum of their 256-thread block counts, and cp_pack_batch() processes all of them in ONE launch.
 * Items of one batch must be independent: views (dgrad / EdgeConv / copies) that feed packs go into an earlier batch.
 * ------------------------------------------------------------------------------------------- */
enum { CP_PACK_GENERIC = 0, CP_PACK_HALO_S = 1, CP_PACK_HALO = 2, CP_PACK_HALO4 = 3, CP_PACK_GEMM = 4,
       CP_PACK_DGRAD_VIEW = 5, CP_PACK_EDGE_VIEW = 6, CP_PACK_COPY_F32 = 7 };
typedef struct CpPackItem {
  int32_t kind;
  int32_t a[9];
  const void* src;
  void* dst;
  const int32_t* row_map;
  uint64_t total;              /* elements = threads of this item */
} CpPackItem;
int cp_pack_item_conv(int dtype, const float* w, int Cout, int Cin, int R, int S, int cin_phys, int transposed, int phase,
                      const int32_t* row_map, int cout_rows, void* packed, CpPackItem* item);      /* cp_pack_conv_weight */
int cp_pack_item_halo(int dtype, const float* w, int Cout, int Cin, int cin_phys, void* packed, CpPackItem* item);  /* cp_pack_conv3x3_halo_weight */
int cp_pack_item_gemm(int dtype, const float* w, int Cout, int Cin, int cin_phys, void* packed, CpPackItem* item);  /* cp_pack_gemm_weight */
int cp_pack_item_dgrad_view(const float* w, int Cout, int Cin, int R, int S, float* wt, CpPackItem* item);          /* cp_weight_dgrad */
int cp_pack_item_edge_view(const float* w, int Cout, int Cin, int mode, float* out, CpPackItem* item);              /* cp_edge_weight_view */
int cp_pack_item_copy_f32(const float* src, float* dst, int count, CpPackItem* item);
int cp_pack_batch(cp_stream_t stream, int dtype, const CpPackItem* items_dev, const uint32_t* block_prefix_dev, int n_items,
                  uint32_t total_blocks);

/* layout plumbing at the boundary: NCHW fp32 image -> channels-last `dtype` (C padded with zeros to
 * Cphys), and channels-last slice -> NCHW fp32 (for `return_img_feats`, init.py:123-124).
 * cp_nhwc_to_nchw_f32: CP_ERR_INVALID for in_coff < 0 or in_coff + C > in_cstride; CP_ERR_RANGE for B > 65535 or more than
 * 65535 channel tiles of 32 (both are grid dimensions). */
int cp_nchw_to_nhwc(cp_stream_t stream, int dtype, const float* in, void* out, int B, int C, int H, int W,
                    int Cphys);
int cp_nhwc_to_nchw_f32(cp_stream_t stream, int dtype, const void* in, float* out, int B, int C, int H, int W,
                        int in_cstride, int in_coff);

/* Input side on the device (next-row N3; reference bop_dataset_pytorch.py:385-391 ToTensor + Normalize): uint8
 * (B,H,W,3) crop -> (x/255 - mean)/std -> channels-last `dtype` with Cphys channels (zero padded).  mean3/std3 are
 * HOST pointers to 3 floats. */
int cp_u8hwc_to_nhwc_norm(cp_stream_t stream, int dtype, const uint8_t* in, void* out, int B, int H, int W, int Cphys,
                          const float* mean3, const float* std3);

/* Input side, second half of row N3: the data loader's RoI crops (bop_dataset_pytorch.py:132-145 get_roi with resize_method
 * crop_square_resize :55-91 or crop_resize :94-108, i.e. zero-padded window + cv2.resize) for a whole batch from full uint8 images
 * (n_img, H, W, C <= 4) resident in device memory.  windows (device, B x 6 int32): x1, y1, x2, y2, roi_w, roi_h -- roi pixel
 * (ry, rx) = image pixel (y1 + ry, x1 + rx) inside [max(x1,0), min(x2,W)) x [max(y1,0), min(y2,H)), zero elsewhere; the roi is resized
 * to crop x crop with cv2's 8-bit INTER_NEAREST (0) / INTER_LINEAR (1) arithmetic.  img_idx (device, B) or NULL when n_img is 1 or B.
 * out: (B, crop, crop, C) uint8, the operand of cp_u8hwc_to_nhwc_norm.  An empty roi gives a zero crop. */
int cp_crop_resize_u8(cp_stream_t stream, const uint8_t* images, int n_img, int H, int W, int C, const int32_t* windows,
                      const int32_t* img_idx, uint8_t* out, int B, int crop, int interpolation);

/* The same crop of ONE BIT of a uint32 plane (next-row N19: cp_render_scene's full_bits / visib_bits): out uint8 (B,crop,crop) is
 * cp_crop_resize_u8's INTER_NEAREST crop -- its window, zero-padding and index arithmetic -- of the mask image
 * (plane[img] >> bit[b]) & 1 ? 255 : 0, which is never stored.  plane uint32 (n_img,H,W); windows, img_idx as above; bit int32 (B) on
 * the device.  An empty roi, or a bit outside 0..31, gives zeros. */
int cp_crop_mask_bits(cp_stream_t stream, const uint32_t* plane, int n_img, int H, int W, const int32_t* windows,
                      const int32_t* img_idx, const int32_t* bit, uint8_t* out, int B, int crop);

/* The loader's third resize_method on the device (next-row N21; csrc/warp_affine.hip; reference bop_dataset_pytorch.py:39-52, 111-145
 * crop_resize_by_warp_affine -> GDR_Net_Augmentation.py:199-240 get_affine_transform -> cv2.warpAffine): B warps of full uint8 images
 * (n_img, H, W, C <= 4) in ONE launch.  inv_mats (device, B x 6 float64): the INVERSE map a00 a01 b0 a10 a11 b1 of each crop -- output
 * pixel (x, y) samples the source at A . (x, y) + b -- inverted on the host as invertAffineTransform does; a row that holds a NaN means
 * "no box": a zero crop.  interpolation: cv2's 8-bit INTER_NEAREST (0) / INTER_LINEAR (1) arithmetic of warpAffine -- coordinates in
 * fixed point (AB_BITS 10, quantised to 1/32 pixel), four taps with 15-bit weights, every tap outside the frame zero on its own
 * (BORDER_CONSTANT 0); the rule is stated in the kernel file's header, the numpy restatement is tests/warp_stages.py.  The caller keeps
 * every output corner's source point within 2^20 pixels of the origin (the int32 fixed point wraps beyond; the Python wrapper refuses).
 * img_idx (device, B) or NULL when n_img is 1 or B.  out: (B, out_h, out_w, C) uint8.  Nothing allocates or synchronises. */
int cp_warp_affine_u8(cp_stream_t stream, const uint8_t* images, int n_img, int H, int W, int C, const double* inv_mats,
                      const int32_t* img_idx, uint8_t* out, int B, int out_h, int out_w, int interpolation);

/* The same warp of ONE BIT of a uint32 plane (cp_render_scene's full_bits / visib_bits): out uint8 (B,out_h,out_w) is
 * cp_warp_affine_u8's INTER_NEAREST warp of the mask image (plane[img] >> bit[b]) & 1 ? 255 : 0, which is never stored.  bit int32 (B)
 * on the device; a NaN row, or a bit outside 0..31, gives zeros. */
int cp_warp_mask_bits(cp_stream_t stream, const uint32_t* plane, int n_img, int H, int W, const double* inv_mats,
                      const int32_t* img_idx, const int32_t* bit, uint8_t* out, int B, int out_h, int out_w);

/* Training-frame augmentation on the device (next-row N13; csrc/augment.hip; reference lm_dataset_pytorch.py:523-541 replace_bg and
 * GDR_Net_Augmentation.py:161-178 build_augmentations): background swap, salt-and-pepper, 5 x 5 motion blur, coarse dropout, 5-tap
 * separable Gaussian and one 256-entry table per channel (Add, Invert, Multiply, Multiply, Contrast composed) for B samples in ONE
 * launch, integer arithmetic only.  frames uint8 (n_img,H,W,3); masks uint8 (n_img,H,W) (non-zero = keep the frame's pixel) and
 * backgrounds uint8 (n_bg,H,W,3), both needed only by samples whose plan asks for the swap (NULL / n_bg = 0 otherwise); out uint8
 * (B,H,W,3).  plan: device blob of cp_augment_plan_bytes(B) bytes, 16-byte aligned, made by checkerpose_amd/augment.py -- 256
 * salt-and-pepper values, then per sample 44 int32 words [key, flags, bg_index, img_index, sp_thresh, drop_thresh, gh, gw, rect x1 y1
 * x2 y2, gauss_w 5 (sum 4096), motion_w 25 (sum 65536), 2 spare] + the table uint8 (3,256); flags: 1 salt-and-pepper, 2 motion,
 * 4 dropout, 8 Gaussian, 16 table, 32 rect (64 x 32 tiles that miss [x1,x2) x [y1,y2) are not computed: out is left as it was there).
 * The steps, their rounding, the border rule (REFLECT_101) and the hash are stated in the kernel's header; the numpy restatement is
 * tests/augment_stages.py.  A sample whose img_index is outside [0, n_img) is not written; a bg_index outside [0, n_bg) means no swap
 * (the Python wrapper refuses both).  H, W >= 5 (four mirrored halo pixels), H, W < 2^15.  Nothing allocates or synchronises;
 * bit-identical for a sample alone or in a batch, at any batch position, with or without a rect. */
size_t cp_augment_plan_bytes(int B);
int cp_augment_frames(cp_stream_t stream, const uint8_t* frames, int n_img, int H, int W, const uint8_t* masks,
                      const uint8_t* backgrounds, int n_bg, const void* plan, int B, uint8_t* out);

/* ---------------------------------------------------------------------------------------------
 * BOP'22 COCO detection / segmentation scores on the device (next-row N15; csrc/coco_eval.hip; reference bop_toolkit
 * scripts/calc_gt_coco.py, scripts/eval_bop22_coco.py, bop_toolkit_lib/pycoco_utils.py and pycocotools' COCOeval as the script drives
 * it).  The rule of every stage is stated in the kernel file's header; the numpy restatement is tests/coco_stages.py.  Nothing
 * allocates or synchronises; every output is bit-identical from call to call and for an item alone or in a batch.
 *
 * cp_coco_pack: masks uint8 (N,H,W), nonzero = set -> bits (N,H,WW) with WW = ceil(W / 32) 32-bit words per row (bit x & 31 of word
 *   x >> 5, zero past W), area (N) and box (N,4) = xmin ymin xmax ymax, -1s for an empty mask.
 * cp_coco_rle_count / cp_coco_rle_write: pycoco_utils.binary_mask_to_rle of the packed masks -- n_runs (N) per mask, then, with
 *   offsets (N + 1 int64, device; the exclusive cumulative sum of n_runs) the concatenated int32 run lengths counts (total).  A mask
 *   whose stretch [offsets[n], offsets[n + 1]) does not lie in [0, total) is not written.
 * cp_coco_mask_iou / cp_coco_box_iou: out[p] (float64) for the listed pairs (P,2) = (detection, ground truth) indices; masks as
 *   cp_coco_pack left them, boxes float64 x y w h (maskApi bbIou).  A pair with an index out of range scores NaN.
 * cp_coco_match: COCOeval.evaluateImg for n_groups (image, category) groups.  offsets: det_off, gt_off, iou_off, n_groups + 1 int32
 *   each, one after the other -- a HOST copy (checked: each starts at 0, ascends and ends at ND / NGT / P, no group keeps more than
 *   CP_COCO_KEEP detections, iou stretch = D x G) and a DEVICE copy (read by the kernel, which checks it again).  A group's detections
 *   are in descending score order, its ground truth in input order; iou holds each group's (D,G) matrix row-major.  det_area (ND),
 *   gt_area (NGT) float64, gt_ignore (NGT) uint8, iou_thrs (CP_COCO_THRS) and area_rng (CP_COCO_AREAS x 2: lo hi) float64 on the
 *   device.  -> dt_match int32 (ND, AREAS, THRS): index of the matched ground truth within its group + 1, 0 = none; dt_ignore uint8 of
 *   that shape; gt_ignore_out uint8 (NGT, AREAS).  scratch: cp_coco_match_scratch_bytes(NGT) bytes, uninitialised.
 * cp_coco_accumulate: COCOeval.accumulate for K categories whose groups are contiguous.  offsets: cat_det_off, cat_gt_off, K + 1 each,
 *   host and device copies as above; det_rank (ND): the detection's position in its group; order (ND): detection indices, each
 *   category's stretch in stable descending score order; max_dets: HOST, CP_COCO_MAXDETS values in [1, CP_COCO_KEEP]; rec_thrs
 *   (CP_COCO_RECS) float64 device.  -> precision float64 (THRS, RECS, K, AREAS, MAXDETS), recall (THRS, K, AREAS, MAXDETS), -1 where a
 *   category has no unignored ground truth.
 * ------------------------------------------------------------------------------------------- */
enum { CP_COCO_THRS = 10, CP_COCO_RECS = 101, CP_COCO_AREAS = 4, CP_COCO_MAXDETS = 3, CP_COCO_KEEP = 100 };
int cp_coco_pack(cp_stream_t stream, const uint8_t* masks, int N, int H, int W, uint32_t* bits, int32_t* area, int32_t* box);
int cp_coco_rle_count(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, int32_t* n_runs);
int cp_coco_rle_write(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, const int64_t* offsets, int32_t* counts,
                      long long total);
int cp_coco_mask_iou(cp_stream_t stream, const uint32_t* det_bits, const int32_t* det_area, const int32_t* det_box, int ND,
                     const uint32_t* gt_bits, const int32_t* gt_area, const int32_t* gt_box, int NG, int H, int W,
                     const int32_t* pairs, int P, double* out);
int cp_coco_box_iou(cp_stream_t stream, const double* det_box, int ND, const double* gt_box, int NG, const int32_t* pairs, int P,
                    double* out);
size_t cp_coco_match_scratch_bytes(int NGT);
int cp_coco_match(cp_stream_t stream, const double* iou, const int32_t* offsets_host, const int32_t* offsets_dev, int n_groups, int ND,
                  int NGT, int P, const double* det_area, const double* gt_area, const uint8_t* gt_ignore, const double* iou_thrs,
                  const double* area_rng, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore_out, void* scratch);
int cp_coco_accumulate(cp_stream_t stream, const int32_t* dt_match, const uint8_t* dt_ignore, const uint8_t* gt_ignore,
                       const int32_t* det_rank, const int32_t* order, const int32_t* offsets_host, const int32_t* offsets_dev, int K,
                       int ND, int NGT, const int32_t* max_dets, const double* rec_thrs, double* precision, double* recall);

/* ---------------------------------------------------------------------------------------------
 * Predicted masks pasted into the frame on the device (row N27; csrc/paste_masks.hip).  The reference never pastes a mask; the rule
 * is this project's own, the integer inverse of the crop window of cp_crop_resize_u8, stated in full at the top of the kernel file
 * and restated in numpy by tests/paste_stages.py: frame pixel (y, x) of mask b is set iff rw, rh > 0, max(x1, 0) <= x < min(x2, W,
 * x1 + rw) (y alike) and seg[((2 (y - y1) + 1) Sh) / (2 rh), ((2 (x - x1) + 1) Sw) / (2 rw)] > CP_SIGMOID_HALF_Z0 (integer division).
 *
 * seg: crop 0's plane of the wanted channel, fp32 logits, Sh x Sw contiguous; seg_bstride: floats between two crops' planes (2 Sh Sw
 *   for the module's (B,2,Sh,Sw) tensor; >= 0).  windows: int32 (B,6) x1 y1 x2 y2 roi_w roi_h on the device, as cp_crop_resize_u8's.
 * cp_paste_masks: -> exactly what cp_coco_pack leaves for the dense pasted masks: bits (B,H,WW), area (B), box (B,4) xmin ymin xmax
 *   ymax (-1s for an empty mask).  Every word is written.  One launch, a workgroup per mask.
 * cp_paste_rle_count / cp_paste_rle_write: -> exactly cp_coco_rle_count / cp_coco_rle_write of those bits, without the bits: n_runs
 *   (B) together with area and box; then, with offsets int64 (B + 1) = 0 and the cumulative sums, counts int32 (total).  A mask whose
 *   offsets do not fit the buffer is not written.  Work proportional to the window.
 * cp_coco_unpack: cp_coco_pack's inverse, bits (N,H,WW) -> masks uint8 (N,H,W) of 0 / 1.
 * No atomics, no scratch, nothing allocates or synchronises; bit-identical for a mask alone or at any batch position.
 * CP_ERR_INVALID: a null pointer, B < 1, seg_bstride < 0, Sh or Sw outside 1..128, H or W outside 1..4096 (cp_coco_unpack: N, H or
 *   W < 1), total < 1; CP_ERR_ALIGN: a pointer not aligned to its element; CP_ERR_RANGE: H * W >= 2^31 - 512, B >= 2^24
 *   (cp_coco_unpack: cp_coco_pack's limits, 2^31 workgroups or more).
 * ------------------------------------------------------------------------------------------- */
int cp_paste_masks(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B, int H,
                   int W, uint32_t* bits, int32_t* area, int32_t* box);
int cp_paste_rle_count(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B, int H,
                       int W, int32_t* n_runs, int32_t* area, int32_t* box);
int cp_paste_rle_write(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B, int H,
                       int W, const int64_t* offsets, int32_t* counts, long long total);
int cp_coco_unpack(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, uint8_t* masks);

/* ---------------------------------------------------------------------------------------------
 * COCO RLE masks decoded on the device (row N29; csrc/rle_unpack.hip; reference pycoco_utils.rle_to_binary_mask).  The inverse of
 * cp_coco_rle_count / cp_coco_rle_write without a dense mask: counts int32 (total) and offsets int64 (N + 1), both on the device, in
 * cp_coco_rle_write's layout -> what cp_coco_pack leaves for the decoded masks.  The rule is stated at the top of the kernel file and
 * restated in numpy by tests/rle_stages.py: with E_j the inclusive ends of mask n's run lengths (64-bit sums), pixel i = x H + y is set
 * iff k = #{ j : E_j <= i } is odd and below the mask's run count; area = the sum of the odd-indexed counts; the box from the runs.
 *
 * cp_coco_rle_unpack: -> bits (N,H,WW), every word written (NULL: area, box and status only, one launch), area (N), box (N,4) xmin
 *   ymin xmax ymax (-1s for an empty mask), status (N): 0 ok; 3 the mask's offsets do not fit [0, total] (no count is read); else 1 a
 *   negative count; else 2 the counts sum to more than H W.  A mask with a nonzero status gets all-zero bits, area 0, a box of -1s.
 *   ends_scratch: cp_coco_rle_unpack_scratch_bytes(total) bytes, uninitialised (the inclusive ends, int32).  The stretches of two
 *   masks must not overlap.  Nothing allocates or synchronises; integer arithmetic only, no atomics; bit-identical for a mask alone
 *   or at any batch position.
 * CP_ERR_INVALID: a null pointer (counts and ends_scratch may be NULL when total == 0; bits may be NULL), N, H or W < 1, total < 0;
 *   CP_ERR_ALIGN: a pointer not aligned to its element; CP_ERR_RANGE: H * W >= 2^31 - 4096, N >= 2^24, total >= 2^31, 2^31
 *   workgroups or more.
 * ------------------------------------------------------------------------------------------- */
size_t cp_coco_rle_unpack_scratch_bytes(long long total);
int cp_coco_rle_unpack(cp_stream_t stream, const int32_t* counts, const int64_t* offsets, int N, int H, int W, long long total,
                       int32_t* ends_scratch, uint32_t* bits, int32_t* area, int32_t* box, int32_t* status);

/* ---------------------------------------------------------------------------------------------
 * hipGraph helpers: capture the launch sequence of one forward (everything above is capture-safe:
 * no allocation, no synchronisation) and replay it with one call.
 * ------------------------------------------------------------------------------------------- */
int cp_graph_begin_capture(cp_stream_t stream);
int cp_graph_end_capture(cp_stream_t stream, void** graph_exec_out);
int cp_graph_launch(void* graph_exec, cp_stream_t stream);
int cp_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* CHECKERPOSE_HIP_H */
