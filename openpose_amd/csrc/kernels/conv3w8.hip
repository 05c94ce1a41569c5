// conv3w8.hip -- 3x3 convolution: the persistent 512 x {128, 96} halo implicit GEMM of conv3w.hip
// with 8 waves of 64 positions x ALL output channels instead of 16 waves of 64 x 64.
//
// Why: the conv3w K loop is bound by LDS fragment reads, not by the MFMAs or the barrier
// (tools/conv3w_probe.hip ablations, 64 frames x 46x82, cin 384: 197 us as built, 194 without the
// mid-unit barrier, 174 without MFMAs, 138 without fragment reads).  With 16 waves of 64 x 64 every
// weight (B) fragment is read by 8 waves and every halo (A) fragment by 2: 8 ds_read_b128 per 16
// MFMAs.  Here a wave owns 64 positions x BN channels (acc 128 VGPRs at 2 waves per SIMD): per tap
// MF = 4 A + NF = 8 B fragments for 32 MFMAs, 25 % fewer LDS reads per MFMA, and the next tap's
// B fragments stream in during taps 0 and 1 of a K unit (fbE / fbO alternate; tap 2 re-reads the
// next unit's tap-0 B into fbE after its last MFMAs), the A fragments two steps ahead.
//
// Same tile, operands, LDS layout, K order and epilogue arithmetic as conv3w_kernel / conv3p_kernel,
// so outputs are bit-identical to them.  Schedule per K unit u = (chunk c, tap row ky), as conv3w:
//     tap 0, tap 1, [wait own DMA of unit u+1; s_barrier], tap 2, [issue DMA of unit u+2];
// fragments of unit u+1 are read during tap 2 (certified by the mid-unit barrier).
//
// lgkmcnt: per tap, step i (position fragment i) issues A(t, i+2) (for i >= 2: the next tap's A
// fragments 0 / 1) and, in taps 0 / 1, the next tap's B fragments 2i, 2i+1; the waits (kWait) are
// counted from that fixed issue order (no other LDS traffic inside the K loop).
#include "conv.h"

#include <algorithm>

#include "../common.h"
#include "conv3_dev.h"

namespace opk {

namespace {

using namespace conv3dev;

constexpr int k8_BM = kConvPersistBM, k8_HR = kConvPersistHR, k8_NW = 8;

// Unit u+2's DMA right after the mid-unit barrier (a third of a unit more lead) instead of after
// tap 2: the split 96- and 64-output tiles (measured 3-3.5 % faster per launch, round 6,
// profiles/round6/split_dma_early/); the 128-output tiles spill 26-30 VGPRs with it (1.5x slower)
// and the fp16 tiles keep their measured schedule.  Dev A/B builds: OPK8_DMA_EARLY 0 never, 1 always.
#ifndef OPK8_DMA_EARLY
#define OPK8_DMA_EARLY 2
#endif
#ifndef OPK8_ABLATE   // dev probe only (tools/conv3w_probe.hip): 1 no mid-unit barrier, 2 no MFMAs,
#define OPK8_ABLATE 0  // 3 no fragment reads, 4 no DMA after the prologue, 5 no MFMAs in tap 1 of
                       // each unit (a third fewer, replaced by VALU adds), 6 the same with nothing
                       // issued in their place, 7 no halo DMA / 8 no weight DMA after the
                       // prologue (timing only, wrong results)
#endif
#if OPK8_ABLATE == 3
#define OPK8_DSR(dst_, addr_, off_) asm volatile("; no read %1" : "=v"(dst_) : "v"(addr_))
#else
#define OPK8_DSR(dst_, addr_, off_)                                                           \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst_) : "v"(addr_), "i"(off_))
#endif

// POOL: the 2x2 / stride-2 max pool that follows the conv (pool2 / pool3 of BODY_25,
// pose_deploy.prototxt:70-87,149-166) fused into the epilogue: a tile is 6 virtual rows starting
// at an odd row, one position in (p0 = (6m + 1) VW + 1), so every pooling window lies inside one
// tile with its column pair in lanes (2k, 2k+1) of a fragment; the lanes take the horizontal max
// through a DPP swap, the first row of each window stores it into the pooled image, and after a
// workgroup barrier the second row's lanes read it back, take the max and store.  The full-size
// conv output is never written.
// MX: the activation as max(t, t*m) (ConvArgs::actmax; conv3_dev.h act_pick)
// BST: one destination, epilogue stores through a buffer resource (ConvArgs::bufst)
typedef unsigned int opk8_u4 __attribute__((ext_vector_type(4)));
#ifndef OPK_FAULT_POOL
#define OPK_FAULT_POOL 0
#endif

// SPLIT: split precision (ConvArgs::split, conv.h): K runs chunk-major over three products per
// input chunk c -- virtual chunk 3c + k: k = 0 x_hi w_lo, 1 x_hi w_hi, 2 x_lo w_hi -- so the hi
// halo of a chunk is staged once for two products (k = 1 issues no halo DMA and reads k = 0's
// slot; hi halos live in slot 0, lo halos in slot 1) and the w_hi tap rows once for two (k = 2
// stages no weights: k = 1 left them in its slots), in the order of conv3_kernel<..., SPLIT>;
// the epilogue writes hi = fp16(v) and lo = fp16(v - hi) of v = act(acc * wscale + bias) --
// bit-identical to conv3_kernel's split instantiations.
// split-precision pooling (POOL && SPLIT): of two (hi, lo) fp16 pairs of 8 channels, keep per
// channel the one with the larger hi + lo (exact in fp32), the first (h1, l1) on ties -- the rule
// of maxpool2_split_kernel (pool.hip), whose raster-order scan this reproduces window-wise
__device__ __forceinline__ void opk8_pair_max(uint4& h1, uint4& l1, const uint4& h2, const uint4& l2)
{
    uint32_t* a = reinterpret_cast<uint32_t*>(&h1);
    uint32_t* al = reinterpret_cast<uint32_t*>(&l1);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(&h2);
    const uint32_t* bl = reinterpret_cast<const uint32_t*>(&l2);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float2_t fa = __builtin_convertvector(__builtin_bit_cast(half2_t, a[w]), float2_t) +
                            __builtin_convertvector(__builtin_bit_cast(half2_t, al[w]), float2_t);
        const float2_t fb = __builtin_convertvector(__builtin_bit_cast(half2_t, b[w]), float2_t) +
                            __builtin_convertvector(__builtin_bit_cast(half2_t, bl[w]), float2_t);
        const uint32_t m = (fb.x > fa.x ? 0x0000ffffu : 0u) | (fb.y > fa.y ? 0xffff0000u : 0u);
        a[w] = (a[w] & ~m) | (b[w] & m);
        al[w] = (al[w] & ~m) | (bl[w] & m);
    }
}

template <int BN, int NB, bool POOL, bool MX, bool BST, bool SPLIT>
__global__ __launch_bounds__(64 * k8_NW, 1) void conv3w8_kernel(const ConvArgs a)
{
#define OPK8_XHI false
#include "conv3w8_kernel_body.h"
#undef OPK8_XHI
}

// XHI: the non-pooled split instantiations over a source without a lo twin (Conv3Query::xhi: every
// channel read was written by an fp16 layer): two products per chunk, x_hi w_lo then x_hi w_hi --
// the third product (x_lo w_hi, which reused the w_hi rows) and the lo DMA stream are gone; the
// sums equal the three-product kernel's over a zero twin (the dropped terms are exact zeros)
template <int BN, int NB, bool MX, bool BST>
__global__ __launch_bounds__(64 * k8_NW, 1) void conv3w8x_kernel(const ConvArgs a)
{
    constexpr bool POOL = false, SPLIT = true;
#define OPK8_XHI true
#include "conv3w8_kernel_body.h"
#undef OPK8_XHI
}

#undef OPK8_DSR

}  // namespace

void launch_conv3w8(const ConvArgs& args, const Conv3Plan& p, hipStream_t stream)
{
    OPK_CHECK_ARG(p.family == Conv3Family::conv3w8, "conv3w8: 96 or k x 128 output channels, 3x3, one aligned slice");
    OPK_CHECK_ARG(p.grid >= 1 && p.grid <= 1024, "persistent grid exceeds the sink");
    OPK_CHECK_ARG((args.pool != 0) == p.pool, "conv3w8 + pool: even H, W and strips, 64 / 128k outputs, border 1");
    OPK_CHECK_ARG(!args.split || ((args.in_lo || p.xhi) && args.dst_lo[0]), "conv3w8 split: lo twins");
    OPK_CHECK_ARG(!p.xhi || (args.split && !p.pool && p.bn != 64), "conv3w8: no hi-only instantiation");
    ConvArgs b = conv3_planned_args(args, p);
    // buffer-resource epilogue stores (BUFST=0: pointer stores, A/B): one destination (pooled:
    // the pooled padded image)
    const int Hd = p.pool ? b.H / 2 + 2 : b.H + 2 * b.border, Wd = p.pool ? b.W / 2 + 2 : b.W + 2 * b.border;
    b.bufst = b.ndst == 1 && conv_bufst_fits(b.frames, Hd, Wd, b.dst_cs[0]) && dev_switch("BUFST", 1) != 0;
    // n-blocks by XCD (W8_NBX=1, dev A/B): measured neutral in both precisions (round 6,
    // profiles/round6/r6c: split 104.0 vs 104.1 ms, fp16 33.6 vs 33.6 ms per 130-frame forward),
    // so the m-tile-major order stays the default
    b.nbx = p.nb > 1 && p.grid % 8 == 0 && dev_switch("W8_NBX", 0) != 0;
    const bool mx = b.actmax != 0, bs = b.bufst != 0, sp = b.split != 0;
    bool launched = false;
    // the hi-only instantiations: BN 96 / 128, NB 1 / 2 / 4, not pooled
#define OPK8X_TRY(BN_, NB_, MX_, BS_)                                                           \
    if (!launched && p.xhi && p.bn == BN_ && p.nb == NB_ && mx == MX_ && bs == BS_) {           \
        note_launch("%s,%d,%d,split,xhi>", p.name, (int)MX_, (int)BS_);                         \
        hipLaunchKernelGGL((conv3w8x_kernel<BN_, NB_, MX_, BS_>), dim3((unsigned)p.grid),       \
                           dim3(64 * k8_NW), 0, stream, b);                                     \
        launched = true;                                                                        \
    }
#define OPK8X_TRY4(BN_, NB_) \
    OPK8X_TRY(BN_, NB_, true, true) OPK8X_TRY(BN_, NB_, true, false)                            \
    OPK8X_TRY(BN_, NB_, false, true) OPK8X_TRY(BN_, NB_, false, false)
    OPK8X_TRY4(128, 4) OPK8X_TRY4(128, 2) OPK8X_TRY4(128, 1) OPK8X_TRY4(96, 1)
#undef OPK8X_TRY4
#undef OPK8X_TRY
#define OPK8_TRY(BN_, NB_, P_, MX_, BS_, SP_)                                                    \
    if (!launched && p.bn == BN_ && p.nb == NB_ && p.pool == P_ && mx == MX_ && bs == BS_ && sp == SP_) { \
        note_launch("%s,%d,%d%s>", p.name, (int)MX_, (int)BS_, SP_ ? ",split" : "");             \
        hipLaunchKernelGGL((conv3w8_kernel<BN_, NB_, P_, MX_, BS_, SP_>), dim3((unsigned)p.grid), \
                           dim3(64 * k8_NW), 0, stream, b);                                     \
        launched = true;                                                                        \
    }
#define OPK8_TRY3(BN_, NB_, P_, MX_) \
    OPK8_TRY(BN_, NB_, P_, MX_, true, true) OPK8_TRY(BN_, NB_, P_, MX_, true, false)             \
    OPK8_TRY(BN_, NB_, P_, MX_, false, true) OPK8_TRY(BN_, NB_, P_, MX_, false, false)
#define OPK8_TRY2(BN_, NB_, P_) OPK8_TRY3(BN_, NB_, P_, true) OPK8_TRY3(BN_, NB_, P_, false)
    OPK8_TRY2(128, 4, true) OPK8_TRY2(128, 2, true) OPK8_TRY2(64, 1, true) OPK8_TRY2(128, 1, true)
    OPK8_TRY2(128, 4, false) OPK8_TRY2(128, 2, false) OPK8_TRY2(128, 1, false) OPK8_TRY2(96, 1, false)
    OPK8_TRY2(64, 1, false)
#undef OPK8_TRY2
#undef OPK8_TRY3
#undef OPK8_TRY
    OPK_CHECK_ARG(launched, std::string("no instantiation of ") + p.name);
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
