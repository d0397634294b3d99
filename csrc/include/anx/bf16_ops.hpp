// anx/bf16_ops.hpp — bf16 MFMA kernels of the full-AlexNet extension (conv_bf16.hip) and the
// full-network engine (full_engine.cpp). Activations are bf16 NHWC, accumulation fp32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "anx/device.hpp"
#include "anx/knobs.hpp"
#include "anx/ops.hpp"
#include "anx/shapes.hpp"

namespace anx {
namespace hip {

struct OutViewB {
  __bf16* base;
  int Hb, Wb, Cb;
  int h_off, w_off, c_off;
};

struct ConvPlanB {
  int N, Hp, Wp, C, K, F, S, groups;
  int Ho, Wo, Cg, Kg, kdim, kpad, kpad_n, variant, vec8;
  int taps8;  // C%8 != 0 (conv1): each filter row's F*C contiguous bf16 cut into 8-element units,
              // the last shifted back to end at F*C (overlap zero-weighted) -> 16-B gathers
};

uint16_t f32_to_bf16_bits(float f);
ConvPlanB make_conv_plan_bf16(int N, int Hp, int Wp, int C, int K, int F, int S, int groups);
size_t packed_weight_elems_bf16(const ConvPlanB& p);
void pack_conv_weights_bf16(const ConvPlanB& p, const float* w_kcff, std::vector<uint16_t>& packed,
                            std::vector<int>& koff);
// Split-K for the fully-connected layers (1x1 "convs" with M = batch): ksplit K slices write fp32
// partial slabs [ksplit][M][K] to ws, splitk_reduce_bf16 sums them + bias (+ReLU) into the output.
struct SplitK {
  int ksplit = 1;
  float* ws = nullptr;
};
int fc_split_k(const ConvPlanB& p);  // chosen slice count (1 = no split)
hipError_t splitk_reduce_bf16(const float* ws, int ksplit, int M, int K, const float* bias, bool relu, OutViewB out,
                              float* out_f32, hipStream_t s);
// out_f32 != nullptr: write fp32 (contiguous [M][K]) instead of the bf16 view (final logits).
// glds (Knobs::bf16_glds): 128x128 vec8 layers (conv2-5, FC) run the LDS-DMA ring with 2 (default) or
// 3 slots, 0 = the register-staged kernel (A/B).
// ran_slots (optional): set at the launch to the kernel that ran, 2 / 3 = the LDS-DMA ring with that many
// slots, 0 = the register-staged kernel of p.variant.
hipError_t conv2d_bf16(const ConvPlanB& p, const void* x, const void* wpacked, const int* koff, const float* bias,
                       OutViewB out, float* out_f32, bool relu, hipStream_t s, SplitK split = {}, int glds = 2,
                       int* ran_slots = nullptr);
// Wide-tile kernel (conv_bf16_big.hip): 1 workgroup per CU, 8 waves over a 256-row tile, LDS-DMA
// double buffer, 16x16x32 MFMA, LDS-transposed epilogue with 16-B stores. Same packed weights / koff
// as conv2d_bf16 (vec8, non-taps8 plans; the koff table is recomputed in arithmetic); bf16 output
// only. cfg (BM x BN, waves, LDS stages): 0 = 256x256 8w 2, 1 = 256x128 8w 2, 2 = 256x96 8w 2,
// 3 = 128x128 4w 2, 4 = 128x96 4w 2, 5 = 256x128 8w 3, 6 = 128x128 4w 3, 7 = 128x96 4w 3,
// 8 = 256x64 8w 3 (FC); 0, 3, 4 read both k-steps' fragments ahead of their MFMAs (PIPE), 9-11 are
// those three without it (A/B); 12 / 13 = 256x256 / 256x128 ping-pong (two staggered 4-wave
// groups; A 2 / B 3 stages; conv only).
int conv_bf16_big_cfgs();
constexpr int kConvBf16BigCfgs = 17;  // == conv_bf16_big_cfgs() (static_assert in conv_bf16_big.hip); knob range
bool conv_bf16_big_ok(const ConvPlanB& p, int cfg, const OutViewB& out);
// The config a cost model of wave quantization picks for this launch (-1: none applies).
int pick_bf16_big_cfg(const ConvPlanB& p, const OutViewB& out, int cus = 256);
// split.ws set (groups == 1): fp32 partial slabs [ksplit][M][Kg] into split.ws, K split ksplit ways
// (no bias / ReLU; then splitk_reduce_bf16, which also serves an fp32 result at ksplit 1). `out` is
// then only validated. ran_cfg (optional): set at the launch to the config that ran (a ping-pong config asked
// for slabs runs as its plain twin).
hipError_t conv2d_bf16_big(const ConvPlanB& p, int cfg, const void* x, const void* wpacked, const int* koff,
                           const float* bias, OutViewB out, bool relu, hipStream_t s, SplitK split = {},
                           int* ran_cfg = nullptr);
// Fully-connected layer plan on the wide-tile kernel (cfg -1: not applicable).
struct BigFc {
  int cfg, ksplit;
};
// cfg >= 0 forces that wide-tile config (knob bf16_fc_cfg; -1 = cfg 8, the measured default).
constexpr int kMaxFcSplit = 16;
// min_kt: K tiles per split-K slice at least this many (knob bf16_fc_minkt)
BigFc pick_bf16_big_fc(const ConvPlanB& p, int cus = 256, int cfg = -1, int min_kt = 4);
hipError_t maxpool_bf16(const void* x, int N, int H, int W, int C, int F, int S, OutViewB out, hipStream_t s);
// tile (Knobs::bf16_lrn_tile): 1 = the generic LDS-tile kernel even where the C = 256 wave kernel applies (A/B).
hipError_t maxpool_lrn_bf16(const void* x, int N, int H, int W, int C, int F, int S, int size, float alpha,
                            float beta, float k, LrnMode mode, OutViewB out, hipStream_t s, int tile = 0);
hipError_t f32_to_bf16(const float* x, void* y, size_t n, hipStream_t s);
// Conv1 polyphase input (space-to-depth by the stride 4) fused with the bf16 conversion:
// y[n][i][j][(rh*4+rw)*3+c] = x[n][4i+rh][4j+rw][c] (0 past the image), y = [N, ceil(H/4), ceil(W/4), 48].
hipError_t f32_to_bf16_s2d4(const float* x, void* y, int N, int H, int W, hipStream_t s);
// Conv1 on the polyphase image as a persistent row-band kernel (conv1_bf16_ring.hip): x' [N,57,57,48]
// bf16, weights packed by pack_conv1_ring_weights from the polyphase fp32 filters [96][48][3][3]
// (conv1_ring_weight_bytes() bytes), bias + ReLU (relu must be true), bf16 NHWC out (55x55x96 view).
void pack_conv1_ring_weights(const float* w_k48_33, std::vector<uint16_t>& out);
size_t conv1_ring_weight_bytes();
// f32_input: x is the fp32 NHWC image [N,227,227,3] (space-to-depth + bf16 conversion inside the
// kernel, no polyphase copy); else the polyphase bf16 image of f32_to_bf16_s2d4.
// pool_out: also max-pool 3x3/2 into this 27x27x96 view (pool1). With f32_input and one workgroup
// per image (N >= cus) the pool runs in the kernel's epilogue and `out` is NOT written (the 55x55
// map never reaches HBM); otherwise Conv1 writes `out` (dense 55x55x96) and maxpool_bf16 follows.
// ran (optional): set at the launch to the segment count (workgroups per image) and whether pool1 ran in the
// kernel's epilogue.
struct RingRan {
  int segs = 0;
  bool pool = false;
};
hipError_t conv1_bf16_ring(const void* x, int N, const void* wpacked, const float* bias, OutViewB out, bool relu,
                           hipStream_t s, int cus = 256, bool f32_input = false, const OutViewB* pool_out = nullptr,
                           RingRan* ran = nullptr);
// The fp32-image form reading the byte image [N,227,227,3] instead (nm.C == 3; x may start at any byte address):
// the loader decodes with fmaf(float(b), nm.sc[c], nm.of[c]) in registers, no float copy of the input exists.
// Same pool_out / ran contract and the same bits as decode_u8 + conv1_bf16_ring(f32_input = true).
hipError_t conv1_bf16_ring_u8(const uint8_t* x, const U8Norm& nm, int N, const void* wpacked, const float* bias,
                              OutViewB out, bool relu, hipStream_t s, int cus = 256, const OutViewB* pool_out = nullptr,
                              RingRan* ran = nullptr);

}  // namespace hip

// Full AlexNet (extension): the reference's Blocks 1-2 followed by the AlexNet tail
// Conv3 3x3/1 p1 (256->384) -> ReLU -> Conv4 (384->384) -> ReLU -> Conv5 (384->256) -> ReLU ->
// MaxPool 3/2 -> FC6 9216->4096 -> ReLU -> FC7 4096->4096 -> ReLU -> FC8 4096->classes.
struct FullWeights {
  // KCFF conv weights / [out][in] FC weights (FC6 input order = NHWC flatten of 6x6x256) + biases
  std::vector<float> w[8], b[8];
};
void full_weight_shapes(int classes, int groups2, size_t wn[8], size_t bn[8]);

// Which kernels FullEngine's last forward launched (its last chunk), written at the launch sites from host
// state only; a layer that has not run yet has a null name.
struct FullPathRecord {
  // Conv1: "ring_f32_pool" (row-band kernel on the fp32 image, pool1 in its epilogue), "ring_f32", "ring" (the
  // same kernel on the polyphase bf16 image), "tiles" (implicit GEMM on the polyphase image) or "taps8" (direct
  // 11x11/4 gathers); segs = workgroups per image of the ring forms (0 otherwise). A byte forward whose ring kernel
  // loaded the bytes itself (last_input "u8_ring") reports "ring_u8_pool" / "ring_u8"; one that decoded first
  // ("u8_decode") reports the float form that then ran.
  const char* conv1 = nullptr;
  int conv1_segs = 0;
  // Conv2-5, FC6-8: "big" (conv_bf16_big.hip, id = config), "glds" (LDS-DMA ring, id = slots) or "staged"
  // (register-staged, id = tile variant); splitk = K slices (1: no split)
  struct Gemm {
    const char* kernel = nullptr;
    int id = -1, splitk = 0;
  } gemm[7];
};

// One call of the full model, as a value: what goes in, what comes out, and which head runs on the logits.
//  * Input: x is [rows,227,227,3] on the device, fp32, or bytes (u8) from any byte address. A byte b of channel c
//    means fmaf(float(b), scale[c], offset[c]) (cpu::decode_u8; set_input_norm, default 1/255, 0), and the logits and
//    every tap equal those of the float call fed the decoded image, bit for bit. With the row-band Conv1 on the image
//    (bf16_conv1 2) and Knobs::bf16_u8 that kernel loads the bytes ("u8_ring": no float copy of the input exists);
//    everywhere else hip::decode_u8 writes the launch chunk as fp32 into a workspace and the float path runs
//    unchanged ("u8_decode"). The first byte call that needs the workspace allocates it (chunk-sized, freed with the
//    engine), never inside a stream capture: warm up once before capturing a graph. No other call allocates.
//  * k == 0, the plain forward: logits [rows,classes] fp32 device.
//  * k > 0, the classifier head: idx int32 [N][k] and prob fp32 [N][k] device, the k most likely classes of each image
//    and their probabilities; logits (nullable) as above, the bits the plain forward writes (logits nobody asked for
//    go to a workspace of the engine). Launch chunks advance the outputs by n * k. Where FC8 went through split-K
//    slabs the head kernel reduces them itself with FC8's bias in place of splitk_reduce_bf16 (Knobs::bf16_head; 0:
//    the reduce writes the logits and the head runs on those); where FC8 writes fp32 directly the head runs on the
//    logits. last_head() tells.
//  * views == 0: N = rows, ranked by logit (cpu::softmax_topk is the definition). views = V in 1 .. kMaxViews: x holds
//    rows = N * V images, image-major (row i * V + v is view v of image i), and idx / prob rank the mean of each
//    image's V softmax rows (cpu::softmax_topk_views; by probability, so V = 1 is not views == 0). A launch chunk then
//    holds whole images: the chunk step is the largest multiple of V the engine's chunk holds.
//  * labels != null, the evaluation head in place of the classifier head (cpu::softmax_eval is the definition; a call
//    has one head, so idx and prob stay null): labels int32 [N] on the device, one per image, k > 0 the top-k
//    threshold, and at least one of rank int32 [N], nll fp32 [N], pred int32 [N], stats uint64 [kEvalStats] and
//    confusion uint32 [classes][classes] on the device, each nullable. views as above (0: ranked by logit, and then
//    classes <= kSoftmaxEvalMaxK). The head runs where the classifier head runs: on FC8's split-K slabs plus bias with
//    Knobs::bf16_head, else on written logits; logits is nullable as for the classifier head. Launch chunks advance
//    labels, rank, nll and pred by the chunk's images; stats and confusion are shared by all chunks (and by every
//    lane that is handed the same ones): integer sums, so the totals do not depend on the order of arrival.
//  * mark: record the engine's mark event on the stream once Conv2 + Pool2/LRN of the first chunk are enqueued (about
//    half of the forward), for wait_mark.
struct FullCall {
  const void* x = nullptr;
  bool u8 = false;
  int rows = 0;
  float* logits = nullptr;
  bool mark = false;
  int k = 0;
  int* idx = nullptr;
  float* prob = nullptr;
  int views = 0;
  const int* labels = nullptr;
  int* rank = nullptr;
  float* nll = nullptr;
  int* pred = nullptr;
  uint64_t* stats = nullptr;
  uint32_t* confusion = nullptr;
};

class FullEngine {
 public:
  FullEngine(const FullWeights& w, int classes, int max_batch, int groups2 = 1, LrnMode lrn = LrnMode::DivN,
             const Knobs& k = default_knobs());
  FullEngine(const FullEngine&) = delete;
  FullEngine& operator=(const FullEngine&) = delete;
  // Runs the layer chain as `c` describes (FullCall above): the only way in. hipErrorInvalidValue, before any launch or
  // event creation, when check(c) gives a reason.
  hipError_t run(const FullCall& c, hipStream_t s);
  // Null, or why run() refuses `c` (a static string): the one statement of the limits on k, views, rows and the
  // pointers (full_engine.cpp), which the C ABI reports word for word.
  const char* check(const FullCall& c) const;
  // The part of check() that needs no engine: what the evaluation head's fields rule out among themselves (labels
  // with idx / prob, outputs without labels, labels without k or without an output). Null for every call that names
  // none of those fields, so for such calls check()'s reasons and their order are what they were.
  static const char* check_eval(const FullCall& c);
  void set_input_norm(const float* scale, const float* offset);  // byte input: three values each
  // What the head of the last call read: "slabs" (it reduced FC8's split-K slabs), "logits" (written logits), null
  // when the last call had no head (k == 0). Recorded at the launch from host state.
  const char* last_head() const { return head_; }
  // How the last call's input reached Conv1: "f32", "u8_ring", "u8_decode"; null before the first. Recorded at
  // the launch site from host state.
  const char* last_input() const { return input_; }
  // Makes `s` wait for the mark event the last call with FullCall::mark recorded, which staggers free-running lanes
  // (AlexNetFull.forward_async) by half a forward.
  hipError_t wait_mark(hipStream_t s) const {
    return mark_ ? hipStreamWaitEvent(s, mark_.get(), 0) : hipErrorInvalidValue;
  }
  int classes() const { return classes_; }
  int max_batch() const { return max_batch_; }
  Knobs& knobs() { return k_; }  // read at every launch (bf16_glds, bf16_big)
  // Debug / numerics taps: copy the bf16 activation buffer `i` of the last forward (images of its
  // last chunk; N <= chunk) to dst on stream s. i: 0 conv1 [N,55,55,96], 1 pool1 window
  // [N,31,31,96], 2 conv2 [N,27,27,256], 3 pool2+LRN window [N,15,15,256], 4 conv3 window
  // [N,15,15,384], 5 conv4 window [N,15,15,384], 6 conv5 [N,13,13,256], 7 pool5 [N,9216],
  // 8 fc6 [N,4096], 9 fc7 [N,4096]. Returns the element count per image (0 for a bad i).
  size_t tap(int i, int N, void* dst, hipStream_t s) const;
  const FullPathRecord& last_path() const { return path_; }

 private:
  HipEvent mark_;
  struct Layer {
    int C, K, F, S, groups;
    DevBuf<uint16_t> wp;  // bf16 packed for tile variant `key`
    DevBuf<int> koff;
    DevBuf<float> bias;
    int key = -1;
    std::vector<float> host;  // KCFF fp32 (re-pack when the tile variant changes)
  };
  // head: FC8 of a call with a head, the call narrowed to the launch chunk at hand (its rows and outputs). Where the
  // layer ends in split-K slabs and Knobs::bf16_head is set, run_head() takes them in place of the reduce.
  hipError_t conv(Layer& L, int N, int Hp, int Wp, const void* x, hip::OutViewB out, float* out_f32, bool relu,
                  hipStream_t s, const FullCall* head = nullptr);
  // The head kernel of launch chunk `ch` (views or not) on its rows at src: FC8's ksplit slabs, slab_stride floats
  // apart, plus bias; or with ksplit 1 and no bias the chunk's written logits. Records last_head().
  hipError_t run_head(const FullCall& ch, const float* src, int ksplit, size_t slab_stride, const float* bias,
                      hipStream_t s);
  hip::U8Norm norm_{3, {1.f / 255.f, 1.f / 255.f, 1.f / 255.f}, {0.f, 0.f, 0.f}};  // byte input: scale / offset
  DevBuf<float> xdec_;             // byte input decoded to fp32 (u8_decode), chunk_ images, allocated on first need
  const char* input_ = nullptr;    // last_input()
  const char* head_ = nullptr;     // last_head()
  DevBuf<float> hlog_;             // classify: a launch chunk's logits [chunk_][classes] when the caller takes none
  Layer L_[8];
  FullPathRecord path_;
  Knobs k_;
  int classes_, max_batch_, chunk_;
  int cus_ = 256;  // compute units (the wide-tile kernel's cost model)
  LrnMode lrn_;
  bool poly1_ = false;  // Conv1 as a stride-1 3x3 conv over the 48-channel polyphase image (ANX_FULL_CONV1)
  DevBuf<uint16_t> w1ring_;  // Conv1 weights packed for conv1_bf16_ring (poly1_ only)
  // The bf16 activation buffers, chunk_ images each, in tap()'s order. kActs is the one table of their sizes:
  // the constructor's allocations and memsets and tap() derive from it.
  enum Act { kC1, kQ2, kC2, kQ3, kQ4, kQ5, kC5, kF6, kF7, kF8, kXb, kNumActs };
  struct ActSpec {
    size_t elems;  // per image
    bool window;   // zero-bordered window: zeroed once, kernels write the interior only
  };
  static const ActSpec kActs[kNumActs];
  DevBuf<uint16_t> act_[kNumActs];
  void* a(Act i) const { return act_[i].get(); }
  DevBuf<float> ws_;  // split-K partial slabs of the FC layers (sized for every batch <= chunk_)
};

}  // namespace anx
