// conv.h -- implicit-GEMM convolution on gfx950 MFMA (fp16 operands, fp32 accumulate).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace opk {

// Activation layout everywhere in the net: NHWC fp16 with a one-pixel zero border,
// [frames][H+2][W+2][cs] ("padded image"), cs = channel stride of the buffer.
// GEMM view of a conv over such images:
//   M = frames * H * (W+2) virtual positions (the two extra columns per row are computed and
//       discarded: every 3x3 tap is then a constant shift of the whole tile),
//   N = output channels, K = taps * cin_pad (tap-major, channels inner, 32-channel chunks).
constexpr int kConvMaxDst = 6;
constexpr int kConvBK = 64;

struct ConvArgs {
    const uint16_t* in;   // fp16 bits, padded image
    int in_cs, in_coff;   // channel stride and first channel of the input slice
    int cin_pad;          // channels read per tap (multiple of 32)
    int ntaps;            // 9 (3x3) or 1 (1x1 / pre-packed)
    int tapoff[9];        // position offset of each tap from the window's top-left position
    int ksteps;           // ceil(ntaps * cin_pad / 64)
    const uint16_t* w;    // [cout_pad][ksteps*64] fp16 bits
    const float* bias;    // [cout]
    const float* slope;   // [cout] PReLU slopes (act == 2)
    int act;              // 0 none, 1 ReLU, 2 PReLU
    int frames, H, W;     // interior size (input and output share it)
    int M;                // frames * H * (W+2)
    int cout;
    int ndst;
    uint16_t* dst[kConvMaxDst];
    int dst_cs[kConvMaxDst], dst_coff[kConvMaxDst];
    float* out32;         // optional NCHW fp32 [frames][out32_c][H][W]
    int out32_c, out32_coff;
    int sw, nstrips;      // conv3 only: strip width and count (set from the plan: conv3_planned_args)
    float rcp[3];         // conv3 only, set from the plan: 1/((H+2)(sw+2)), 1/(sw+2), 1/nstrips
    int wide;             // conv3 only, set by launch_conv3: 16-byte epilogue stores allowed (CONV3_WIDE)
    int prio;             // conv3 persistent: s_setprio(1) around each unit's MFMAs (CONV3P_PRIO)
    void* sink;           // conv3 persistent variant: >= kConv3SinkBytes of scratch (masked stores)
    int cus;              // compute units the conv was planned for.  No kernel and no launcher reads
                          // it back (the grid is the plan's); conv3_query, for the probe tools, does
    int border;           // zero border of the padded images (conv3 / conv_image; 0 means 1)
    int actmax;           // conv3w / conv3w8: every negative-side multiplier (1 none, 0 ReLU, the
                          // PReLU slopes) lies in [0, 1], so t > 0 ? t : t*m == max(t, t*m) for
                          // every finite t (the epilogue's 2 VALU per value become 1); set by the host
    int bufst;            // conv3w: one destination whose extent is < 2^31 bytes -- epilogue stores
                          // through a buffer resource (set by launch_conv3w)
    int pool;             // conv3w8: 2x2/2 max pool fused into the epilogue; dst[0] is the pooled
                          // padded image [frames][H/2+2][W/2+2][cs] (Conv3Plan::pool)
    int nbx;              // conv3w8, several n-blocks: XCD x computes n-block x % NB only, so an
                          // XCD's L2 holds one n-block's weights (set by launch_conv3w8)
    // Split precision (NetHip precision OPK_PRECISION_SPLIT; conv3_kernel only): every activation
    // x is held as two fp16 images, hi = fp16(x) and lo = fp16(x - hi) (in_lo / dst_lo: the lo
    // twins, same layout and offsets), and every weight w as w_hi = fp16(w), w_lo = fp16(w - w_hi).
    // The K loop runs three products per 32-channel input chunk, chunk-major -- x_hi * w_lo,
    // x_hi * w_hi (the same staged hi halo), x_lo * w_hi (the w_hi tap rows of the product
    // before, still in their weight slots: conv3w8 stages no weights for it) (weights packed
    // [cout_pad/BN][2 * cin_pad/32][ky][kx][BN][32]: the w_hi chunks, then the w_lo chunks) --
    // each product exact in fp32, so only the fp32 summation and the dropped x_lo * w_lo term
    // (~2^-22 relative) separate the result from an fp32 convolution.  The weights are packed
    // scaled by a power of two per layer, w' = w * 2^e with max |w'| in [2^14, 2^15), so w_lo is
    // a normal fp16 number (a He-init weight of ~0.03 would otherwise leave w - w_hi in fp16's
    // subnormal range, ~8 bits); the epilogue multiplies the sums by wscale = 2^-e before the
    // bias (exact: a power of two).  Kernels: conv3_kernel, conv3w8_kernel and conv_image_kernel
    // (SPLIT instantiations; the fp16 instantiations ignore wscale).
    int split;
    const uint16_t* in_lo;
    uint16_t* dst_lo[kConvMaxDst];
    float wscale;
    int small;            // small-batch tiles asked for.  No kernel and no launcher reads it back (the
                          // launchers take a Conv3Plan); conv3_query, for the probe tools, does
    int pbn;              // conv3s only, set by conv3_planned_args: the n-block of the weight packing
};
// the product of a split virtual chunk (3c + k) that reads w_lo: k = 0 (the order above; dev A/B
// builds: OPK_SPLIT_WLO_K=1, the round-6 order x_hi w_hi, x_hi w_lo, x_lo w_hi, every product
// staging its weights)
#ifndef OPK_SPLIT_WLO_K
#define OPK_SPLIT_WLO_K 0
#endif

// conv3.hip: 7x7, 3x3 and 1x1, input halo staged once per 32-channel chunk over a "virtual image" of
// column strips (sw interior columns each).  Tile BM x BN = 256 x 128 / 96 (<= 80 KB LDS, two
// workgroups per CU, or 136 KB, one), 512 x 64 for cout <= 64; optional fp32 NCHW output (out32).
// Weights packed [cout_pad/BN][cin_pad/32][ky][kx][BN][32] (BN = conv3_pack_bn).  Reads padded positions down to -1
// and the whole row past the last one: buffers carry zeroed guards (kConvGuardTail positions).
constexpr int kConvGuardTail = 1024;   // positions
constexpr size_t kConv3SinkBytes = (size_t)1024 * 1024 * 16;   // 1024 lanes x 1024 workgroups x 16 B
// the tile of the persistent kernels (conv3p, conv3w, conv3w8): positions and halo rows (the
// kernels keep bias / slopes in LDS: 688 halo rows where the 16-wave conv3_kernel has 704)
constexpr int kConvPersistBM = 512, kConvPersistHR = 688;

// ---- conv_plan.cpp: the one decider of which kernel runs a conv, on which tile, strips and grid --
// Plain host code (no HIP calls): NetHip's planner (once per input shape: its launch list,
// opk_net_conv_plan and opk_net_conv_kernels read that one answer) and the probe tools ask
// conv3_plan / conv3_runs and nothing else decides; the launchers below take the plan they are given.
//
// Positions are decoded by float-reciprocal division in the kernels (Strips::map), exact below
// 2^24: a launch's last position (tile and halo overhang included) must fit
constexpr long kConvMaxPositions = 1L << 24;
inline bool conv_positions_fit(long last) { return last < kConvMaxPositions; }
// epilogue stores through a buffer resource: positions x channel stride of the destination (guards
// included) within the 31-bit offsets of the raw buffer range check
inline bool conv_bufst_fits(int frames, int Hp, int Wp, int cs)
{
    return ((long)frames * Hp * Wp + kConvGuardTail) * cs * 2 < (1L << 31) - 4096;
}
// n-block of conv3's weight packing (cout only -- and, for 1x1 convs, the CONV1_TILE switch)
int conv3_pack_bn(int cout, int ks);

enum class Conv3Family { conv3, conv3p, conv3w, conv3w8, conv3s };

// what the decision depends on (no pointers: fillable before any device memory exists)
struct Conv3Query {
    int frames, H, W, cout, cin_pad, ntaps;
    int border;                   // zero border of the net's padded images (<= 0 means 1)
    int ndst, dst_cs[kConvMaxDst], dst_coff[kConvMaxDst];   // (pool requested: the pooled image's)
    bool out32;                   // an fp32 NCHW output
    bool split;
    // split only: the source has no lo twin -- no channel the conv reads has a split writer (a
    // precision schedule's fp16 -> split boundary, NetHip).  conv3_query: ConvArgs::in_lo == NULL
    bool xhi;
    bool pool;                    // 2x2/2 max pool in the epilogue requested
    bool small;                   // small-batch tiles requested (NetHip small-batch mode)
    bool sink;                    // scratch for the persistent kernels' masked stores
    int cus;                      // compute units; 0: no persistent kernel
};
Conv3Query conv3_query(const ConvArgs& a);

struct Conv3Plan {
    Conv3Family family;
    // template parameters of the instantiation (those the geometry fixes)
    int bm, bn, hr, tapu, minb, ks, nw;
    int nb;                       // conv3w8: n-blocks (cout / 128)
    int pbn;                      // n-block of the weight packing (conv3s reads conv3's packing)
    bool pool;                    // conv3w8 POOL epilogue (false though requested: not supported)
    bool split;
    // the hi-only split instantiation (template parameter XHI of conv3_kernel / conv3w8_kernel:
    // x_hi w_lo + x_hi w_hi, no lo halo) runs: asked for (Conv3Query::xhi, dev switch SPLIT_XHI
    // not 0) and the tile has one (conv_tiles.h: conv3_tile_has_xhi, conv3w8_tile_has_xhi).  false
    // though asked: the three-product kernel, which needs a (zero) lo twin on the source
    bool xhi;
    int sw, nstrips, VW;         // strip width and count, virtual row VW = sw + 2 border
    long total;                   // virtual positions: frames * nstrips * (H + 2 border) * VW
    long grid;                    // workgroups launched
    // the planner's measure of how far the geometry fills the chip: tiles of the GEMM's
    // M = frames * H * (W + 2 border) positions times n-blocks (the grid also covers the border
    // rows and the strips' shared columns: a few per cent more; persistent grids stop at cus)
    long workgroups;
    bool fits;                    // conv_positions_fit: false -> fewer frames per launch (conv3_runs)
    float rcp[3];                 // 1/((H + 2B) VW), 1/VW, 1/nstrips (ConvArgs::rcp)
    // launch-log name: the whole instantiation for conv3_kernel / conv3s_kernel (hi-only:
    // "...,split,xhi>"), up to the parameters the plan fixes for the persistent kernels
    // ("conv3w8_kernel<BN,NB,POOL"; hi-only: "conv3w8x_kernel<BN,NB", logged "...,split,xhi>").
    // These are log names, not symbols: conv3s_kernel<...> and "...,xhi>" are instantiations of
    // conv3_kernel, conv3w8x_kernel<...> of conv3w8_kernel (XHI = true)
    char name[64];
};
// Every decision switch of the halo kernels is read here (opk_dev_set; per call, so tests compare
// variants in one process): CONV3_SMALL, CONV3_W16, CONV3_PERSIST, CONV1_TILE, CONV1_N64W16,
// CONV3W8_64, SPLIT_W8, CONV3W8N, CONV3W (0 / not), CONV3W8, CONV3S_MAX, CONV7S_BIG, SPLIT_XHI,
// SPLIT_XHI_W8.
// When a switch is read.  A *decision* switch -- those above, the ones NetHip::dispatch reads
// (CONV1_FUSED, HEAD_FUSE, HEAD_FUSE_SPLIT, POOL_FUSE), GRID_CUS and EPI_MAX -- is read when NetHip
// plans an input shape and holds for that shape's plan: forwards replay the planned launches and
// ask nothing again.  A new net, set_conv, set_precision* and set_small_batch re-plan; flipping a
// decision switch on a net that already holds a plan for a shape leaves that shape's forwards as
// they were.  The launchers' own instantiation flags (BUFST, W8_NBX, CONV3W=2, CONV3_WIDE,
// CONV3P_PRIO, CONV3P_ASMR, CONV3P_WIDE, HEAD_PERSIST, CONV_IMAGE_WIDE, CONV_IMAGE_STAGE) and
// LAUNCH_LOG are read per forward.  Throws for sizes no kernel covers
// and for a plan whose tile is not on the list of instantiations (conv_tiles.h): "no instantiation of <name>".
// only: a probe tool's choice among the persistent kernels of a conv that supports it (-1: the
// product rule); plan.family differs from it when the conv does not.
Conv3Plan conv3_plan(const Conv3Query& q, int only = -1);
// The launches of a conv over q.frames frames: one run of whole frames per launch, as few as the
// kernels' position range allows.  One run when the whole batch's plan fits; else the fewest even
// runs (ceil(frames / runs) frames each, the last one the rest) whose every run fits.  Each run
// carries the plan of ITS frame count: a run with fewer tiles may fall into another tile branch
// (another halo, so another strip count) than the whole batch.  Nothing else walks runs.
struct Conv3Run {
    int f0, frames;               // first frame and frame count
    Conv3Plan plan;
};
std::vector<Conv3Run> conv3_runs(const Conv3Query& q);
// the small-batch rule: conv3s when the product geometry gives fewer than cus workgroups and
// conv3s supports the conv and gives more, but no more than kConv3sMaxPerCu per CU (measured: the
// 64 x 32 tile is level with the 256-position tiles at 2.8 workgroups per CU and 1.8x slower at 5.7;
// the 7x7 tiles keep the cap: at 1 - 8 face / hand crops and 1 - 2 COCO frames every forward
// measured faster with it)
constexpr int kConv3sMaxPerCu = 4;
// the larger (128 x 64) 7x7 tile is taken where it gives a workgroup per this many CUs (3x3: two).
// Measured: with two, one COCO frame and two face / hand crops take the 64 x 32 tile, whose
// launched grid (border rows and strip overlap included: 308 / 340 workgroups) no longer fits one
// round on 256 CUs -- 3.62 against 3.17 ms and 2.26 against 2.01 ms per forward
constexpr int kConv7sBigPerCus = 4;
// the arguments a launcher hands its kernel: sw, nstrips, border, rcp and pbn set from the plan
ConvArgs conv3_planned_args(const ConvArgs& a, const Conv3Plan& p);

// launch-log names of the other conv kernels a net's conv can run in (the launchers log them with
// their template arguments; opk_net_conv_kernels reports the bare names)
constexpr char kConvImageKernel[] = "conv_image_kernel";
constexpr char kConv1FusedKernel[] = "conv1_fused_kernel";
constexpr char kConvHeadKernel[] = "conv_head_kernel";

// conv3.hip: the public entry -- checks the arguments against the plan and launches what the plan
// says (it does not plan: the caller's conv3_plan / conv3_runs did).  Families conv3
// and conv3s are conv3_kernel itself: 7x7, 3x3 and 1x1 tiles of 8 / 16 waves and, for forwards too
// small to fill the chip with those, 3x3 (any border) and 7x7 (border >= 3) tiles of 4 waves
// (64 x 32 or 128 x 64; logged as conv3s_kernel<...>), bit-identical to the larger ones
void launch_conv3(const ConvArgs& a, const Conv3Plan& p, hipStream_t stream);
// conv3w.hip: the persistent 512 x {128, 96} 3x3 variant with one mid-unit barrier per K unit
void launch_conv3w(const ConvArgs& a, const Conv3Plan& p, hipStream_t stream);
// conv3w8.hip: the same tile with 8 waves of 64 x BN (fewer LDS fragment reads per MFMA)
void launch_conv3w8(const ConvArgs& a, const Conv3Plan& p, hipStream_t stream);

// conv_head.hip: Mconv6 (1x1, n1 = 256 / 512 outputs, act6) -> Mconv7 (1x1, n2 <= 64 outputs) in
// one kernel; the Mconv6 activations never leave the chip.  Input / outputs as ConvArgs (padded
// NHWC fp16 slices, optional fp32 NCHW out32).  w6: [cin_pad/32][n1][32] fp16; w7: packed by
// conv_head_pack_w7 ([n2 <= 32 ? 32 : 64][n1], K permuted within 32-channel blocks); b7 zero-padded
// to 64 floats; b6 / s6 [n1].
struct HeadArgs {
    const uint16_t* in;
    int in_cs, in_coff, cin_pad;
    const uint16_t* w6;
    const float *b6, *s6;
    int act6;
    const uint16_t* w7;
    const float* b7;
    int n1, n2;
    int frames, H, W;
    int ndst;
    uint16_t* dst[kConvMaxDst];
    int dst_cs[kConvMaxDst], dst_coff[kConvMaxDst];
    float* out32;
    int out32_c, out32_coff;
    int cus;              // > 0: persistent grid of this many workgroups (conv_head.hip)
    int actmax;           // Mconv6's negative-side multipliers all in [0, 1] (ConvArgs::actmax)
    // split precision (ConvArgs::split): the input as (in, in_lo) fp16 pairs, w6 packed
    // [2][cin_pad/32][n1][32] (w_hi block, then w_lo), w7 [2][n2p][n1] (each K-permuted), both
    // scaled by 2^e per layer (sums times wscale6 / wscale7 before the bias); Mconv6's activation
    // is split into (hi, lo) on chip and Mconv7 runs x_hi w_hi + x_lo w_hi + x_hi w_lo; outputs
    // hi to dst, lo to dst_lo
    int split;
    const uint16_t* in_lo;
    uint16_t* dst_lo[kConvMaxDst];
    float wscale6, wscale7;
};
bool conv_head_supported(int n1, int n2, int cin_pad);
void conv_head_pack_w7(uint16_t* dst, const uint16_t* w7 /* [n2][n1] */, int n1, int n2);
void launch_conv_head(const HeadArgs& a, hipStream_t stream);

// First conv (3 input channels, 3x3, cout <= 64) straight from the fp32 NCHW input [frames][3][H][W]
// (conv_image.hip); weights [cout_pad][64], K order (ky*3 + kx)*3 + ci.
void launch_conv_image(const ConvArgs& a, const float* image, hipStream_t stream);

// conv1_1 (3 -> 64) + act -> conv1_2 (64 -> 64) + act -> 2x2/2 max pool in one persistent kernel
// (conv1_fused.hip).  img: fp32 NCHW [frames][3][H][W]; w1: [64][64] (K order (ky*3+kx)*3+ci);
// w2: conv3 packing for BN = 64; bias/slope arrays zero-padded to 128; out: the pooled padded NHWC
// fp16 image [frames][OH+2][OW+2][out_cs] (slice at out_coff).  H and W even.
struct Conv1FusedArgs {
    const float* img;
    int frames, H, W;
    const uint16_t* w1;
    const float *b1, *s1;
    int act1;
    const uint16_t* w2;
    const float *b2, *s2;
    int act2;
    uint16_t* out;
    int out_cs, out_coff, OH, OW;
    int actmax;           // both convs' negative-side multipliers in [0, 1] (ConvArgs::actmax)
};
bool conv1_fused_supported(int H, int W, int cout1, int cout2);
void launch_conv1_fused(const Conv1FusedArgs& a, int workgroups, hipStream_t stream);

// 2x2 stride-2 max pool with Caffe ceil sizing, padded NHWC fp16 -> padded NHWC fp16.
// split precision: the lo twins of input and output; the pooled pair is the (hi, lo) pair of the
// largest hi + lo (exact in fp32)
void launch_maxpool2_split(uint16_t* out, uint16_t* out_lo, const uint16_t* in, const uint16_t* in_lo,
                           int frames, int H, int W, int C, int OH, int OW, hipStream_t stream,
                           int border);
void launch_maxpool2(uint16_t* out, const uint16_t* in, int frames, int H, int W, int C, int OH,
                     int OW, hipStream_t stream, int border = 1);

}  // namespace opk
