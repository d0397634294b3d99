// anx/ops.hpp — layer operators: CPU reference kernels and HIP (gfx950) launchers.
//
// Layouts: activations NHWC (channel fastest, the reference's per-image
// HWC plus a batch axis); conv weights KCFF `((k*C+c)*F+fh)*F+fw` as the reference stores them
// (v1_serial/src/layers_serial.cpp:70). The fast MFMA path repacks KCFF once into a
// GEMM-friendly [K][F*F*C] image (see ConvPlan) — the reference re-uploads weights every call
// (v4_mpi_cuda/src/alexnet_mpi_cuda.cu:176-191); we keep them resident.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "anx/knobs.hpp"
#include "anx/shapes.hpp"

namespace anx {

// ----------------------------------------------------------------------------------------
// CPU reference kernels (V1 / V2 compute, golden oracle). Parity:
// serialConvLayer/ReluLayer/MaxPoolLayer/LRNLayer (v1_serial/src/layers_serial.cpp:37-175).
// ----------------------------------------------------------------------------------------
namespace cpu {
// y[N,Ho,Wo,K] = conv(x[N,H,W,C], w[K,C/g,F,F]) + b ; zero padding P, stride S, groups g.
// `pad_top`/`pad_bottom` override P on the H axis (row tiles: only global edges are padded).
void conv2d(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int C, int K, int F,
            int S, int P, int groups, bool relu, int pad_top = -1, int pad_bottom = -1);
void relu(float* x, size_t n);
void maxpool(const float* x, float* y, int N, int H, int W, int C, int F, int S);
void lrn(const float* x, float* y, int N, int H, int W, int C, int size, float alpha, float beta, float k,
         LrnMode mode);
// Byte image -> float: y[i] = fmaf(float(x[i]), scale[i % C], offset[i % C]), one fused multiply-add in fp32.
// THE definition of the byte input's meaning: hip::decode_u8 and the byte loader of the one-kernel Conv1
// evaluate the same expression, so every path is comparable bit for bit. The reference has no byte input.
void decode_u8(const uint8_t* x, float* y, size_t n, int C, const float* scale, const float* offset);
// Top-k class probabilities of M rows of K logits. THE definition of the classifier head: hip::softmax_topk
// computes the same logits bits and the same indices. Per row m:
//   z[c]   = bias[c] + src[0][m][c] + ... + src[ksplit-1][m][c] over the split-K slabs src[s] = src + s *
//            slab_stride (floats), fp32 adds in exactly that order (splitk_reduce_bf16's); without a bias the sum
//            starts from slab 0, so logits pass through with their bits (ksplit 1, bias null);
//   idx[j] = the k best classes by value descending, then index ascending; float comparison, so -0.0 and +0.0 tie
//            (a NaN ranks below everything, as -inf does, so a row of any values yields k distinct indices);
//   prob[j] = exp(z[idx[j]] - max) / sum_c exp(z[c] - max) in fp32 (unspecified for a row holding a NaN or
//            whose maximum is infinite).
// 1 <= k <= min(K, kMaxTopK). idx int32 [M][k], prob [M][k], logits_out (nullable) [M][K] = the bits of z.
// The reference ends at Block 2's LRN and has no classifier head.
constexpr int kMaxTopK = 16;
void softmax_topk(const float* src, int ksplit, size_t slab_stride, const float* bias, int M, int K, int k, int* idx,
                  float* prob, float* logits_out);
// The view-averaging head: N images of V views each, rows [N * V][K] image-major (row i * V + v is view v of image
// i). THE definition of hip::softmax_topk_views. Per row, z is reduced as in softmax_topk and
//   p_v[c]  = exp(z[c] - max) / sum_c exp(z[c] - max)           (softmax_topk's expressions, fp32)
// per image
//   pbar[c] = ((p_0[c] + p_1[c]) + ... + p_{V-1}[c]) / float(V)  (fp32, adding in view order)
//   idx[j]  = the k best classes by pbar descending, then index ascending (a NaN ranks with -inf)
//   prob[j] = pbar[idx[j]].
// The ranking is by probability, not by logit: with V = 1 the probabilities are softmax_topk's bits, but classes whose
// probabilities underflow to the same value tie here and go to the lower index, where softmax_topk still tells
// their logits apart. 1 <= V <= kMaxViews, 1 <= k <= min(K, kMaxTopK). idx int32 [N][k], prob [N][k], probs_out
// (nullable) [N][K] = pbar, logits_out (nullable) [N * V][K] = the bits of z. The reference has no classifier head.
constexpr int kMaxViews = 32;
void softmax_topk_views(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                        int* idx, float* prob, float* probs_out, float* logits_out);
// The evaluation head: the model held to labels. THE definition of hip::softmax_eval. The rows are those of
// softmax_topk_views ([N * V][K], reduced from slabs (+ bias) in softmax_topk's order, into logits_out when given),
// and V == 0 means one row per image (N rows). Per image i with label y = labels[i], the score row r is
//   V == 0: z, the logits (softmax_topk's rule: ranked by logit);   V >= 1: pbar, softmax_topk_views' expressions,
// ordered by value descending, then index ascending, a NaN as -inf (the rule of both heads above). Then
//   pred[i] = the class that ranks first (idx[i][0] of the head above on the same rows);
//   rank[i] = the number of classes that rank before y: rank < k exactly when y is among the k classes that head
//             returns, and idx[i][rank[i]] == y there;
//   nll[i]  = V == 0: logf(S) - (z[y] - m), m the row maximum and S = sum_c expf(z[c] - m) as softmax_topk sums it
//             (finite where the probability underflows, +inf for a -inf label logit);
//             V >= 1: -logf(pbar[y]), the log loss of the averaged prediction (+inf where pbar[y] is 0).
// A label outside 0 .. K-1 (the -1 padding of a last batch) marks an ignored image: rank = -1, nll = 0, pred as
// above, and nothing is counted. Every other image adds into the caller-zeroed counters
//   stats[kEvalCount] += 1, stats[kEvalTop1] += rank == 0, stats[kEvalTopK] += rank < k,
//   stats[kEvalNll] += eval_nll_q32(nll)      (fixed point, 32 fraction bits: mean loss = stats[3] / 2^32 / stats[0])
//   confusion[y][pred] += 1                   (uint32 [K][K])
// which are integer sums, so the totals are the same bits whatever order images, chunks, lanes and workgroups finish
// in. rank, nll, pred, stats, confusion and logits_out are each nullable. 0 <= V <= kMaxViews, 1 <= k <= min(K,
// kMaxTopK). nll of a row holding a NaN is unspecified, as prob is. The reference has no classifier head.
enum { kEvalCount = 0, kEvalTop1 = 1, kEvalTopK = 2, kEvalNll = 3, kEvalStats = 4 };
// q(x) = uint64(double(min(x, 1024)) 2^32 + 0.5): a NaN, or anything not < 1024 (+inf included), counts as 1024, and
// a value below 0 (-logf of a mean that rounded a last bit above 1) as 0. At most 2^-33 off per image.
__host__ __device__ inline uint64_t eval_nll_q32(float nll) {
  const float c = !(nll < 1024.f) ? 1024.f : nll > 0.f ? nll : 0.f;
  return static_cast<uint64_t>(static_cast<double>(c) * 4294967296.0 + 0.5);
}
void softmax_eval(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                  const int* labels, int* rank, float* nll, int* pred, uint64_t* stats, uint32_t* confusion,
                  float* logits_out);
}  // namespace cpu

// One source image of resize_crop_u8: H x W x 3 bytes, HWC, rows `pitch` bytes apart (pitch >= 3W), from any byte
// address; and its box in its own pixels: origin (y0h, x0h) in HALF pixels (a centred crop of odd slack is exact),
// size bh x bw pixels, inside the image.
struct ImageDesc {
  const uint8_t* ptr;
  int H, W;
  int64_t pitch;
  int y0h, x0h, bh, bw;
};
// The limits of resize_crop_u8, checked before any memory is touched: 1 <= OH, OW <= 512; per image a pointer,
// 1 <= H, W <= 16384, pitch >= 3W, bh, bw >= 1, 0 <= y0h, y0h + 2 bh <= 2H (likewise x), bh <= 16 OH, bw <= 16 OW.
// Returns null when all n descriptors pass, else a static message naming the first limit missed.
const char* resize_crop_check(const ImageDesc* d, int n, int OH, int OW);

namespace cpu {
// Antialiased resize + crop of byte images: image i's box resampled onto out[i] (OH x OW x 3 bytes, images
// contiguous) with torch / PIL's antialiased bilinear (triangle) filter in fixed point, horizontal pass first.
// THE definition of the operation (hip::resize_crop_u8 computes the same bytes). With the per-axis 15-bit tap
// weights q of anx/resize_taps.hpp:
//   h[y][ox][c]     = (sum_j q^x_j src[y][j][c] + 64) >> 7          (16 bits, at most 65280)
//   out[oy][ox][c]  = (sum_y q^y_y h[y][ox][c] + 2^22) >> 23        (in [0, 255] without a clamp)
// The descriptors must have passed resize_crop_check. The reference has no resampling: its programs fill floats.
void resize_crop_u8(const ImageDesc* d, int n, uint8_t* out, int OH, int OW);
// The same with mirrored outputs: flip (nullable: none) holds one byte per output, and an output whose byte is
// nonzero is the unflipped output of its descriptor with the columns reversed, out[oy][OW - 1 - ox][c]. Taps,
// rounding and limits are untouched. Descriptors may name the same image more than once (views of one source).
void resize_crop_u8(const ImageDesc* d, const uint8_t* flip, int n, uint8_t* out, int OH, int OW);
}  // namespace cpu

// ----------------------------------------------------------------------------------------
// HIP launchers. All take device pointers and a stream; none allocate or synchronise
// (safe under hipGraph capture). Return hipSuccess or the launch error.
// ----------------------------------------------------------------------------------------
namespace hip {

// Naive one-thread-per-output kernels: the device-side correctness oracle (the shape of the
// reference's convKernel/poolKernel/lrnKernel, v3_cuda_only/src/layers_cuda.cu:20-152).
hipError_t conv2d_direct(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int C,
                         int K, int F, int S, int P, int groups, bool relu, hipStream_t s);
hipError_t relu(float* x, size_t n, hipStream_t s);
hipError_t maxpool_direct(const float* x, float* y, int N, int H, int W, int C, int F, int S, hipStream_t s);
hipError_t lrn_direct(const float* x, float* y, int N, int H, int W, int C, int size, float alpha, float beta,
                      float k, LrnMode mode, hipStream_t s);

// A strided NHWC destination: element (n,h,w,c) of the logical output lands at
// base + ((n*Hb + h + h_off)*Wb + w + w_off)*Cb + c_off + c. Lets producers write straight into
// the zero-bordered input buffer of the next conv (no pad pass) or into a channel slice.
struct OutView {
  float* base;
  int Hb, Wb, Cb;
  int h_off, w_off, c_off;
};

// Implicit-GEMM convolution on f32 MFMA (v_mfma_f32_32x32x2_f32), LDS-staged, fused
// bias + optional ReLU epilogue. The input buffer must already hold the zero padding
// (Hp = H + pads): the kernel performs no bounds checks on reads.
struct ConvPlan {
  int N, Hp, Wp, C;   // padded input dims
  int K, F, S, groups;
  int Ho, Wo;         // output dims
  int Cg, Kg;         // per-group channels / filters
  int kdim;           // F*F*Cg (real)
  int kpad;           // kdim rounded up to BK
  int kpad_n;         // Kg rounded up to BN
  int variant;        // tile configuration id
  int vec4;           // A is gathered in 4-float units (16-B loads)
  int taps4;          // Cg%4 != 0 (conv1, C=3): each filter row's F*C contiguous floats are cut
                      // into 4-float units, the last one shifted back to end at F*C (its
                      // overlap gets zero weight) -> kdim = F*4*ceil(F*C/4), 16-B gathers
};
// force_vec4 / force_scalar: tile variant override for Cg%4==0 / scalar-gather convs (A/B tuning,
// Knobs::force_vec4 / force_scalar; -1 or an invalid id = the heuristic).
ConvPlan make_conv_plan(int N, int Hp, int Wp, int C, int K, int F, int S, int groups, int force_vec4 = -1,
                        int force_scalar = -1);
bool conv_variant_valid(int kind, int id);
// Packed weights: [groups][kpad_n][kpad] with k = (fh*F + fw)*Cg + c (taps4: k = (fh*U + u)*4 + e
// over the 4-float units u of filter row fh); zero padded.
size_t packed_weight_floats(const ConvPlan& p);
// Offset table: [kpad] int32 input offsets (relative to the pixel's window origin), -1 = padding.
size_t koff_ints(const ConvPlan& p);
// Host-side packing (weights come from the host in KCFF order).
void pack_conv_weights_host(const ConvPlan& p, const float* w_kcff, std::vector<float>& packed,
                            std::vector<int>& koff);
hipError_t conv2d_mfma(const ConvPlan& p, const float* x, const float* wpacked, const int* koff,
                       const float* bias, OutView out, bool relu, hipStream_t s);

// Winograd F(m x m, 5x5) for stride-1 5x5 convolutions over a pre-padded input window (winograd.hip):
// m = 3 (7x7 input tiles, 49 points) or m = 4 (8x8, 64 points; Knobs::conv2_tile).
struct WinoPlan {
  int N, Hq, Wq, C, K, groups;
  int Ho, Wo, ty, tx, P;  // output dims, m x m tiles per column/row, total tiles
  int m;                  // output tile side
};
// m = 3: 96 or 48 channels per group and a multiple of 64 filters per group; m = 4: one group, 96
// channels, a multiple of 64 filters (the fused GEMMs' shapes)
bool wino_eligible(int F, int S, int C, int K, int groups, int m = 3);
WinoPlan make_wino_plan(int N, int Hq, int Wq, int C, int K, int groups, int m = 3);
size_t wino_v_floats(const WinoPlan& w);  // V workspace [P][(m+4)^2][C]
size_t wino_u_floats(const WinoPlan& w);  // transformed weights [(m+4)^2][K][C/groups]
// U[(ab*groups + g)*Kg + k][c] = (G g G^T)[a][b] in fp64, rounded once.
void wino_transform_weights_host(const WinoPlan& w, const float* w_kcff, std::vector<float>& u_kcff);
hipError_t wino_input(const WinoPlan& w, const float* x, float* V, hipStream_t s);
// Pool1 (3x3 / 2 max) fused with the input transform: V straight from the conv1 output c1 [N][H1][W1][C]
// (conv1 row c1_lo first). Window row R is pool1 row q_lo + R (zero outside [0, Hp)), window column c is
// pool1 column c - P (zero outside [0, Wp)); every non-zero window row must be computable from c1's rows.
// Bit-identical to maxpool + wino_input. C % 32 == 0, Wq <= 31, and the pooling must be 3x3 / stride 2
// (pool_F, pool_S; anything else returns hipErrorInvalidValue: the kernel's walk is written for 3/2).
hipError_t wino_pool_input(const WinoPlan& w, const float* c1, int H1, int W1, int q_lo, int Hp, int Wp, int P,
                           int c1_lo, float* V, hipStream_t s, int pool_F = 3, int pool_S = 2);
// Input transform of a conv2 window whose pool1 pixels were written by conv1_fused_pool: straddling
// pixels take max(window, p1) (p1: [N][Hp][Wp][C], image 0 = tile-numbering image n_off of the Conv1
// launch with ty1 x tx1 tiles per image). Window row R is pool1 row q_lo + R, column c pool1 column c - P.
// pg: channels per workgroup, 32 (31 KiB of LDS, 512 threads) or 16 (15.5 KiB, 256 threads: fits beside a
// Conv1 workgroup of the per-wave-ring kernel, 142 KiB, on one CU; knob conv2_in_pg).
hipError_t wino_window_merge_input(const WinoPlan& w, const float* window, const float* p1, int n_off, int ty1, int tx1,
                                   int q_lo, int Hp, int Wp, int P, float* V, hipStream_t s, int pg = 32);
// Fused batched GEMM + output transform + bias + optional ReLU into `out` (wino_gemm.hpp); Knobs:
// conv2_occ (workgroups per CU cap).
hipError_t wino_conv2(const WinoPlan& w, const float* V, const float* U, const float* bias, OutView out, bool relu,
                      hipStream_t s, const Knobs& k);

// Conv1 (stride 4, C = 3, 8 < F <= 12, no padding) as Winograd F(3x3,3x3) on the polyphase image
// (conv1_wino.hip): 48 polyphase channels, 3x3 output tiles, 25 transform points.
struct Conv1WinoPlan {
  int N, Hin, W, K, F;
  int H1, W1, ty, tx, P;  // output dims, 3x3 tiles per column/row, total tiles
};
bool conv1_wino_eligible(int C, int K, int F, int S, int P, int groups);
Conv1WinoPlan make_conv1_wino_plan(int N, int Hin, int W, int K, int F);
size_t conv1_wino_v_floats(const Conv1WinoPlan& w);  // V workspace [P][25][48]
size_t conv1_wino_u_floats(int K);                   // transformed weights [25][K][48]
void conv1_wino_weights_host(int K, int F, const float* w_kcff, std::vector<float>& u);
// x: [N, Hin, W, 3] image rows; writes conv1 (+bias, optional ReLU) through `out`. Knobs: conv1_occ,
// conv1_band, conv1_fused (1 / 2: the one-kernel form below instead of transform kernel + GEMM).
// *one_kernel (if given) reports which of the two forms was launched.
hipError_t conv1_wino(const Conv1WinoPlan& w, const float* x, float* V, const float* U, const float* bias, OutView out,
                      bool relu, hipStream_t s, const Knobs& k, bool* one_kernel = nullptr);
// The one-kernel form (conv1_fused.hip): the input transform generated in LDS inside the GEMM, each
// workgroup 32 tiles x all 96 filters (V never reaches HBM, U through an LDS-DMA ring). Eligible for
// K == 96.
bool conv1_fused_eligible(const Conv1WinoPlan& w, const OutView& out);
hipError_t conv1_fused(const Conv1WinoPlan& w, const float* x, const float* U, const float* bias, OutView out, bool relu,
                       hipStream_t s);
// The same kernel with pool1 (3x3 / 2 max) in its epilogue: the 55x55 conv1 map never leaves LDS. Pooled
// pixel (py, px) of image n is written to `window` (pool1 image at h_off / w_off, e.g. the conv2 input
// window) by the workgroup owning the window's top-left Conv1 tile; when the window's tiles straddle two
// workgroups' 32-tile ranges (pool1_straddles), that value is the lower workgroup's partial max and the
// upper one's is in p1 [N][Hp][Wp][K]: the consumer takes the max of both (wino_window_merge_input).
// Exact (max in any order), so the merged pool1 map equals conv1_fused + maxpool.
constexpr int kConv1FusedTiles = 32;  // Conv1 tiles per conv1_fused workgroup (raster order)
__host__ __device__ inline bool pool1_straddles(int n, int py, int px, int ty1, int tx1) {
  const int b = n * ty1 * tx1;
  const int gm = b + (2 * py / 3) * tx1 + (2 * px) / 3, gM = b + ((2 * py + 2) / 3) * tx1 + (2 * px + 2) / 3;
  return gm / kConv1FusedTiles != gM / kConv1FusedTiles;
}
bool conv1_fused_pool_eligible(const Conv1WinoPlan& w, const OutView& window, int Hp, int Wp);
hipError_t conv1_fused_pool(const Conv1WinoPlan& w, const float* x, const float* U, const float* bias, OutView window,
                            float* p1, int Hp, int Wp, bool relu, hipStream_t s, int um = 0);
// Whether conv1_wino launches the one-kernel form for this plan, destination and knobs (the one definition:
// the engine asks it before it decides how a byte image reaches Conv1).
bool conv1_wino_one_kernel(const Conv1WinoPlan& w, const OutView& out, const Knobs& k);

// Byte images (uint8 NHWC). A byte b of channel c means fmaf(float(b), sc[c], of[c]) (cpu::decode_u8).
constexpr int kU8MaxC = 16;
struct U8Norm {
  int C;
  float sc[kU8MaxC], of[kU8MaxC];
};
// y[i] = fmaf(float(x[i]), sc[i % C], of[i % C]) for n elements; x may start at any byte address and n may be
// anything (16-B loads where the source is aligned, single bytes before and after).
hipError_t decode_u8(const uint8_t* x, float* y, size_t n, const U8Norm& nm, hipStream_t s);
// The one-kernel Conv1 forms reading the byte image directly (C == 3): the decode happens in the X' loader,
// no fp32 copy of the input exists. Same eligibility, output and bits as decode_u8 + the fp32 forms.
hipError_t conv1_fused_u8(const Conv1WinoPlan& w, const uint8_t* x, const U8Norm& nm, const float* U, const float* bias,
                          OutView out, bool relu, hipStream_t s);
hipError_t conv1_fused_pool_u8(const Conv1WinoPlan& w, const uint8_t* x, const U8Norm& nm, const float* U,
                               const float* bias, OutView window, float* p1, int Hp, int Wp, bool relu, hipStream_t s,
                               int um = 0);

// Antialiased resize + crop of a batch of byte images of different sizes in one launch (resize_crop_u8.hip;
// cpu::resize_crop_u8 is the definition, and the kernel writes the same bytes). `dev` holds the n descriptors in
// device memory (their ptr fields device addresses); `host` is the caller's host copy of the same descriptors: the
// launcher checks every limit on it (resize_crop_check) and sizes the kernel's LDS from it, so the kernel never
// runs on an unvalidated box. Returns hipErrorInvalidValue for a missed limit or a null pointer; n == 0 launches
// nothing. out: n x OH x OW x 3 bytes, from any byte address.
hipError_t resize_crop_u8(const ImageDesc* dev, const ImageDesc* host, int n, uint8_t* out, int OH, int OW,
                          hipStream_t s);
// The same with mirrored outputs (the flip overload of cpu::resize_crop_u8 is the definition): one flag byte per
// output, carried like the descriptors as a device copy the kernel reads and the caller's host copy. Both null: the
// call above, byte for byte (and the same kernel); one null and the other not: hipErrorInvalidValue. The flag is
// uniform over a workgroup and only moves the bytes where the band is assembled in LDS, so resampling, staging and the
// 16-B stores are shared.
hipError_t resize_crop_u8(const ImageDesc* dev, const ImageDesc* host, const uint8_t* flip_dev, const uint8_t* flip_host,
                          int n, uint8_t* out, int OH, int OW, hipStream_t s);

// The classifier head (softmax_topk.hip; cpu::softmax_topk is the definition): one workgroup per row reduces the
// split-K slabs (+ bias) once, keeps the row in LDS, and writes the k best classes and their softmax probabilities;
// logits_out (nullable) receives the reduced row. A row's result depends only on the bits of its logits, not on
// M, the row's position, or whether it came from slabs or a logits array. Rows of more than kSoftmaxTopkLdsRow
// floats are staged in logits_out instead of LDS: without one the call returns hipErrorInvalidValue, as it does
// for k or K out of range and null idx / prob / src. M == 0 launches nothing.
constexpr int kSoftmaxTopkLdsRow = 15 * 1024;
hipError_t softmax_topk(const float* src, int ksplit, size_t slab_stride, const float* bias, int M, int K, int k,
                        int* idx, float* prob, float* logits_out, hipStream_t s);
// The view-averaging head (softmax_topk_views.hip; cpu::softmax_topk_views is the definition): one workgroup per
// image keeps a view's reduced row and the running sum of the views' softmax rows in LDS, loops over the image's V
// consecutive rows (each reduced from slabs (+ bias) or read as logits, as above), divides by V and ranks the mean.
// probs_out (nullable) [N][K] receives the mean row, logits_out (nullable) [N * V][K] the reduced rows. Two rows must
// fit the LDS: K <= kSoftmaxViewsMaxK; that, V outside 1 .. cpu::kMaxViews, k outside 1 .. min(K, kMaxTopK) and null
// src / idx / prob return hipErrorInvalidValue. N == 0 launches nothing. expf is the device's, so the probabilities
// are held to fp64 like the host definition's, not to the host's bits; an image's result depends only on the bits
// of its rows' z, on V and on K.
constexpr int kSoftmaxViewsMaxK = 7680;
hipError_t softmax_topk_views(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K,
                              int k, int* idx, float* prob, float* probs_out, float* logits_out, hipStream_t s);
// The evaluation head (softmax_eval.hip; cpu::softmax_eval is the definition): one workgroup per image keeps the
// score row in LDS (the logits with V == 0; a view's row and the running mean with views, as the view head does),
// finds the first class in one argmax round and the label's rank in one counting pass, and thread 0 adds the image
// into stats / confusion with integer atomics (no float atomics: the totals do not depend on arrival order). rank,
// nll, pred, stats, confusion and logits_out are each nullable. The row(s) must fit the LDS: K <= kSoftmaxEvalMaxK
// with V == 0 (no staging in logits_out as softmax_topk has it), K <= kSoftmaxViewsMaxK with views; that, V outside
// 0 .. cpu::kMaxViews, k outside 1 .. min(K, kMaxTopK) and null src / labels return hipErrorInvalidValue before any
// launch. N == 0 launches nothing. Same pred and the same order as the other two heads on the same rows' bits.
constexpr int kSoftmaxEvalMaxK = kSoftmaxTopkLdsRow;
hipError_t softmax_eval(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                        const int* labels, int* rank, float* nll, int* pred, uint64_t* stats, uint32_t* confusion,
                        float* logits_out, hipStream_t s);

// The fused Winograd GEMM + output transform (wino_gemm.hip). V [P][points][C], U [points][K][C/groups]
// (row = filter), bias + optional ReLU, NHWC store through `out` (Cb, c_off multiples of 4). P tiles of
// 3x3 outputs on a ty x tx grid per image, Ho x Wo outputs. occ: workgroups-per-CU cap (0 = none).
// abl / cfg: 0 / -1 = the production kernel; other ablations and configurations exist only in the
// anx_wgemm A/B build.
hipError_t wino_gemm_conv2(const float* V, const float* U, const float* bias, OutView out, int P, int ty, int tx, int Ho,
                           int Wo, int C, int K, int groups, bool relu, hipStream_t s, int occ = 0, int abl = 0,
                           int cfg = -1);
hipError_t wino_gemm_conv1(const float* V, const float* U, const float* bias, OutView out, int P, int ty, int tx, int Ho,
                           int Wo, int K, bool relu, hipStream_t s, int occ = 0, int abl = 0, int cfg = -1);
// The F(4x4,5x5) form (wino_gemm16.hpp): V [P][64][96], U [64][K][96], P tiles of 4x4 outputs, K % 64 == 0.
// abl 0 = the compiler-scheduled kernel, kConv2SchedAbl = the hand-scheduled slice (knob conv2_sched; bitwise
// identical), other values = A/B-tool probes.
constexpr int kConv2SchedAbl = 64 + 256 + 512;
hipError_t wino_gemm_conv2_f45(const float* V, const float* U, const float* bias, OutView out, int P, int ty, int tx,
                               int Ho, int Wo, int K, bool relu, hipStream_t s, int occ = 0, int abl = 0, int cfg = -1);
// The same GEMM with pool2 (3x3 / 2 max) in its epilogue: the 27x27 conv2 map never reaches HBM. Pooled
// pixel (py, px) of image n goes to pooled [n][Hp][Wp][K] from the workgroup owning the window's top-left
// 4x4 tile (tile (py / 2, px / 2)); when the window's tiles straddle two workgroups' 32-tile ranges
// (pool2_straddles), that value is the lower workgroup's partial max and the upper one's is in p2 (same
// layout): the consumer takes the max of both (lrn_pooled_merge). Exact (max in any order).
constexpr int kConv2PoolTiles = 32;  // Conv2 4x4 tiles per F(4x4,5x5) GEMM workgroup (raster order)
__host__ __device__ inline bool pool2_straddles(int n, int py, int px, int ty2, int tx2) {
  const int gm = n * ty2 * tx2 + (py >> 1) * tx2 + (px >> 1);
  const int gM = gm + ((py & 1) ? tx2 : 0) + (px & 1);
  return gm / kConv2PoolTiles != gM / kConv2PoolTiles;
}
hipError_t wino_gemm_conv2_f45_pool(const float* V, const float* U, const float* bias, float* pooled, float* p2, int P,
                                    int ty, int tx, int Ho, int Wo, int Hp, int Wp, int K, bool relu, hipStream_t s,
                                    int occ = 0, bool sched = false);


// Dynamic LDS bytes that cap a kernel at `wgs` workgroups per CU (160 KiB LDS per CU): the larger of
// `natural` and just over 160 KiB / (wgs + 1). wgs <= 0: `natural`.
size_t occupancy_lds(size_t natural, int wgs);

// Vectorised NHWC max-pool writing through an OutView (C % 4 == 0 required for the fast path).
hipError_t maxpool(const float* x, int N, int H, int W, int C, int F, int S, OutView out, hipStream_t s);
// Fused max-pool + cross-channel LRN (block 2 tail).
hipError_t maxpool_lrn(const float* x, float* y, int N, int H, int W, int C, int F, int S, int size,
                       float alpha, float beta, float k, LrnMode mode, hipStream_t s);
// LRN of a pooled map written by wino_gemm_conv2_f45_pool (C == 256, size 5): pixel (n, py, px) is
// max(pooled, p2) where pool2_straddles(n % sub, ...) (sub: images per GEMM launch, ty2 x tx2 tiles per
// image), pooled alone elsewhere. Bit-identical to maxpool_lrn of the unpooled map. max_wgs > 0 caps the
// grid (knob lrn_wgs: each wave then walks several pixel pairs; same output bits).
hipError_t lrn_pooled_merge(const float* pooled, const float* p2, float* y, int N, int Hp, int Wp, int C, int ty2,
                            int tx2, int sub, int size, float alpha, float beta, float k, LrnMode mode, hipStream_t s,
                            int max_wgs = 0);

// Zero the rows of an NHWC buffer outside [row_lo, row_hi) and the W border (halo buffers).
hipError_t fill(float* x, size_t n, float v, hipStream_t s);
// 16-B-vector copy on exactly `workgroups` workgroups (the ingest probe's stand-in for a collective's
// receive channels: tools/probe_ingest.py). bytes % 16 == 0, both pointers 16-B aligned.
hipError_t channel_copy(void* dst, const void* src, size_t bytes, int workgroups, hipStream_t s);

}  // namespace hip
}  // namespace anx
