// conv3s.hip -- small-tile 3x3 and 7x7 convolutions for forwards of a few frames (NetHip
// small-batch mode).
//
// conv3_kernel's tiles cover 256 or 512 positions by 64 / 96 / 128 outputs: one BODY_25 frame at
// 656 x 368 gives the 46 x 82 stage layers 16 workgroups on a 256-CU chip.  conv3s_kernel is
// conv3_kernel (conv3.hip: the halo of a 32-channel chunk staged once, every tap a constant row
// shift of it, weights as the MFMA's A operand, epilogue straight from registers) with 4 waves
// (2 x 2) on a tile of
//   64 positions x 32 outputs, one K unit per chunk (all 9 taps' weights staged together: a
//       128-channel layer is 4 barriers long, its first two units' loads in flight at once),
//   128 positions x 64 outputs, 3-tap K units (conv3_kernel's schedule; 76 KB of LDS: two
//       workgroups per CU),
// and, for the 7x7 layers of the COCO / MPI / face / hand stages (one crop of 46 x 46 gives
// conv3_kernel<256,...,7> 10 workgroups), the same two tiles with one tap row (7 taps) per K unit:
//   64 x 32 under a 384-row halo (90 KB of LDS), 128 x 64 under a 448-row halo (140 KB),
// chosen by conv3_plan (conv_plan.cpp).  The geometry is in padded positions of any border B
// (VW = sw + 2 B), so the 3x3 tiles also run the 3x3 layers of a 3-pixel-border net.  (A third
// tile, 128 x 128 with single-tap units and two workgroups per CU, measured slower than
// conv3_kernel's tiles wherever the rule picked it; DESIGN.md.)  The weights are read from conv3's
// packing
// [cout_pad/PBN][cin_pad/32][ky][kx][PBN][32]: a tile's n-block is the row range
// [n0 % PBN, n0 % PBN + BN) of every [PBN][32] tap block (BN divides PBN).
//
// Arithmetic: the same MFMA, lane assignment and K order (chunk-major, then tap ky*KS + kx; split
// precision: x_hi w_lo, x_hi w_hi, x_lo w_hi per chunk, each over all taps) as conv3_kernel, so the
// outputs are bit-identical.
#include "conv.h"

#include <algorithm>

#include "../common.h"
#include "conv3_dev.h"

namespace opk {

namespace {

using namespace conv3dev;

constexpr int kS_NW = 4;   // waves per workgroup

// KS: 3 (TAPU 3 or 9) or 7 (TAPU 7: a tap row per unit -- a chunk's 49 taps x 32 outputs are 100 KB)
template <int BM, int BN, int HR, int TAPU, bool SPLIT, int KS = 3>
__global__ __launch_bounds__(64 * kS_NW) void conv3s_kernel(const ConvArgs a)
{
    constexpr int NW = kS_NW, WAVES_N = 2, WAVES_M = NW / WAVES_N;
    constexpr int WROWS = BM / WAVES_M, WN = BN / WAVES_N;   // wave tile WROWS x WN
    static_assert(WROWS % 16 == 0 && WN % 16 == 0, "wave tiles");
    static_assert((KS == 3 && (TAPU == 3 || TAPU == 9)) || (KS == 7 && TAPU == 7), "taps per unit");
    constexpr int MF = WROWS / 16, NF = WN / 16;
    constexpr int KT = KS * KS, UPC = KT / TAPU;  // taps, units per 32-channel chunk
    constexpr int API = HR / 16;                  // halo DMA instructions per block (16 rows each)
    constexpr int AIW = (API + NW - 1) / NW;      // ... per wave, at most
    constexpr int BROWS = TAPU * BN;              // B rows per unit: tap-major, then channel n
    constexpr int BPI = BROWS / 16, BIW = (BPI + NW - 1) / NW;
    constexpr int ASLOT = HR * 4;                 // 16-byte pieces per halo slot
    constexpr int NAS = UPC >= 2 ? 2 : 3;         // halo slots: unit u+2 starts chunk c+2 if UPC == 1
    constexpr int BSLOT = BROWS * 4;
    constexpr int LDS_PIECES = NAS * ASLOT + 3 * BSLOT;
    static_assert(HR % 16 == 0 && BN % 16 == 0, "DMA granularity");
    static_assert(LDS_PIECES * 16 <= 160 * 1024, "LDS budget");
    static_assert(AIW + BIW <= 15, "vm_wait_rt range");
    __shared__ uint4 lds[LDS_PIECES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave - (wave / WAVES_N) * WAVES_N;
    const Strips g(a);
    const int nn = (a.cout + BN - 1) / BN;
    // XCD-aware bijective tile order (see conv3.hip)
    const int nblk = gridDim.x;
    const int xcd = blockIdx.x & 7, qq = nblk >> 3, rr = nblk & 7;
    const int tix = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (blockIdx.x >> 3);
    const int p0 = (tix / nn) * BM;
    const int nb = tix - (tix / nn) * nn;
    const int n0 = nb * BN;
    // the packed n-block (PBN channels) this tile's BN channels lie in, and their first row in it
    const int pbn = a.pbn;
    const int pb = n0 / pbn, r0 = n0 - pb * pbn;

    // ---- DMA lane geometry: 16 rows x 4 pieces per wave instruction --------------------------
    const int lrow = lane >> 2, phys = lane & 3;
    const int cpt = a.cin_pad >> 5;               // 32-channel chunks of the input
    // split precision: three products per input chunk, as conv3_kernel (virtual chunk 3c + k)
    const int cptk = SPLIT ? 3 * cpt : cpt;
    const int U = UPC * cptk;
    const ptrdiff_t dlo = SPLIT ? a.in_lo - a.in : 0;
    // halo row hr = (i*NW + wave)*16 + lrow holds virtual position p0 - (KS/2)*(VW + 1) + hr
    const uint16_t* arow[AIW];
#pragma unroll
    for (int i = 0; i < AIW; ++i) {
        const int hr = (i * NW + wave) * 16 + lrow;
        const int lp = phys ^ (((hr >> 2) & 1) << 1);
        int f, yy, xx, s;
        const long pos = g.template map<false>(p0 - (KS / 2) * (g.VW + 1) + hr, f, yy, xx, s);
        arow[i] = a.in + a.in_coff + pos * a.in_cs + lp * 8;
    }
    // weight row rb = (j*NW + wave)*16 + lrow of a unit: tap rb / BN of the unit, channel rb % BN
    int boff[BIW];
#pragma unroll
    for (int j = 0; j < BIW; ++j) {
        const int rb = (j * NW + wave) * 16 + lrow;
        const int lp = phys ^ (((rb >> 2) & 1) << 1);
        boff[j] = ((rb / BN) * pbn + r0 + rb % BN) * 32 + lp * 8;
    }
    const int ai = (API - wave + NW - 1) / NW;
    const int bi = (BPI - wave + NW - 1) / NW;
    const uint16_t* wbase = a.w + (size_t)pb * (SPLIT ? 2 * cpt : cpt) * KT * pbn * 32;
    // packed chunk of virtual chunk cc_ (split: w_lo chunks follow the w_hi chunks)
#define OPK3S_WCHUNK(cc_) (!SPLIT ? (cc_) : ((cc_) % 3 == OPK_SPLIT_WLO_K ? cpt + (cc_) / 3 : (cc_) / 3))
#define OPK3S_ASLOT(c_) (!SPLIT ? (c_) % NAS : ((c_) % 3 == 2 ? 1 : (UPC == 1 ? 2 * (((c_) / 3) & 1) : 0)))
#define OPK3S_HALO(c_) (!SPLIT || (c_) % 3 != 1)
#define OPK3S_ISSUE(u_)                                                                       \
    do {                                                                                      \
        const int c_ = (u_) / UPC, tu_ = (u_) - c_ * UPC;                                     \
        if (tu_ == 0 && OPK3S_HALO(c_)) {                                                     \
            const int as_ = OPK3S_ASLOT(c_) * ASLOT;                                          \
            const ptrdiff_t ao_ = !SPLIT ? (ptrdiff_t)c_ * 32                                  \
                                         : (ptrdiff_t)(c_ / 3) * 32 + (c_ % 3 == 2 ? dlo : 0); \
            _Pragma("unroll") for (int i_ = 0; i_ < AIW; ++i_)                                \
                if (API % NW == 0 || i_ * NW + wave < API)                                    \
                    __builtin_amdgcn_global_load_lds(                                         \
                        (const void*)(arow[i_] + ao_),                                        \
                        (__attribute__((address_space(3))) void*)(&lds[as_ + (i_ * NW + wave) * 64]), \
                        16, 0, 0);                                                            \
        }                                                                                     \
        const int bs_ = NAS * ASLOT + ((u_) % 3) * BSLOT;                                     \
        const uint16_t* ub_ = wbase + ((size_t)OPK3S_WCHUNK(c_) * KT + tu_ * TAPU) * pbn * 32; \
        _Pragma("unroll") for (int j_ = 0; j_ < BIW; ++j_)                                    \
            if (BPI % NW == 0 || j_ * NW + wave < BPI)                                        \
                __builtin_amdgcn_global_load_lds(                                             \
                    (const void*)(ub_ + boff[j_]),                                            \
                    (__attribute__((address_space(3))) void*)(&lds[bs_ + (j_ * NW + wave) * 64]), \
                    16, 0, 0);                                                                \
    } while (0)

    float4_t acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

    const int r16 = lane & 15, q = lane >> 4;
    // bias and negative-side multiplier (1: identity, 0: ReLU, slope: PReLU) of this lane's
    // output channels (the arrays are zero-padded to a multiple of 128 channels)
    float4_t bv[NF], mv[NF];
    const float neg = a.act == 1 ? 0.f : 1.f;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int ch = n0 + wn * WN + j * 16 + 4 * q;
        bv[j] = *reinterpret_cast<const float4_t*>(a.bias + ch);
        const float4_t sl = *reinterpret_cast<const float4_t*>(a.slope + ch);
        mv[j] = a.act == 2 ? sl : float4_t{neg, neg, neg, neg};
    }
    // (their loads must not be counted by the K loop's vmcnt waits)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    OPK3S_ISSUE(0);
    if (U > 1) OPK3S_ISSUE(1);
    for (int u = 0; u < U; ++u) {
        const int c = u / UPC, t = u - (u / UPC) * UPC;
        // this wave's loads of unit u have landed once only unit u+1's may still be in flight
        vm_wait_rt(u + 1 < U ? bi + (t == UPC - 1 && OPK3S_HALO(c + 1) ? ai : 0) : 0);
        __builtin_amdgcn_s_barrier();
        if (u + 2 < U) OPK3S_ISSUE(u + 2);
        const uint4* As = lds + OPK3S_ASLOT(c) * ASLOT;
        const uint4* Bs = lds + NAS * ASLOT + (u % 3) * BSLOT;
#pragma unroll
        for (int k = 0; k < TAPU; ++k) {
            const int tap = t * TAPU + k;         // ky*KS + kx
            const int ky = tap / KS, kx = tap - KS * (tap / KS);
            half8_t fa[MF], fb[NF];
            const int hoff = ky * g.VW + kx;
#pragma unroll
            for (int i = 0; i < MF; ++i)
                fa[i] = __builtin_bit_cast(half8_t, As[swz64(wm * WROWS + i * 16 + r16 + hoff, q)]);
#pragma unroll
            for (int j = 0; j < NF; ++j)
                fb[j] = __builtin_bit_cast(half8_t, Bs[swz64(k * BN + wn * WN + j * 16 + r16, q)]);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    }
#undef OPK3S_ISSUE
#undef OPK3S_WCHUNK
#undef OPK3S_ASLOT
#undef OPK3S_HALO

    // ---- epilogue straight from registers (conv3_kernel's) -------------------------------------
    // lane (q, r16) of fragment (i, j) holds output channels ch..ch+3 (ch = n0 + wn*WN + j*16 + 4q)
    // of virtual position p0 + wm*WROWS + i*16 + r16; border and out-of-image positions are dropped.
    long prow[MF];
    bool pok[MF];
    const int pbase = p0 + wm * WROWS + r16;
    {   // fragment i is 16 virtual positions after fragment i-1: step the coordinates
        int f, yy, xx, s;
        prow[0] = g.map(pbase, f, yy, xx, s);
        pok[0] = g.interior(yy, xx, s, a.W);
#pragma unroll
        for (int i = 1; i < MF; ++i) {
            if (g.VW > 16) {
                xx += 16;
                if (xx >= g.VW) {
                    xx -= g.VW;
                    if (++yy == g.Hp) {
                        yy = 0;
                        if (++s == g.nstrips) {
                            s = 0;
                            ++f;
                        }
                    }
                }
                const bool in = pbase + i * 16 < g.total;
                prow[i] = in ? (long)(f * g.Hp + yy) * g.Wp + s * g.sw + xx : -1;
                pok[i] = in && g.interior(yy, xx, s, a.W);
            } else {
                int f2, yy2, xx2, s2;
                prow[i] = g.map(pbase + i * 16, f2, yy2, xx2, s2);
                pok[i] = g.interior(yy2, xx2, s2, a.W);
            }
        }
    }
    const int chl = n0 + wn * WN + 4 * q;   // this lane's first channel (fragment j adds 16 j)
    const bool vec = (a.cout & 3) == 0;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const float4_t bj = bv[j], mj = mv[j];
        const int ch = chl + j * 16;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            // (split: the sums of the 2^e-scaled weights times 2^-e, exact; conv.h)
            const float4_t t = (SPLIT ? acc[i][j] * a.wscale : acc[i][j]) + bj;
            const float4_t tm = t * mj;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = t[r] > 0.f ? t[r] : tm[r];
            if (!pok[i] || ch >= a.cout) continue;
            const half2_t h01 = __builtin_convertvector((float2_t){v[0], v[1]}, half2_t);
            const half2_t h23 = __builtin_convertvector((float2_t){v[2], v[3]}, half2_t);
            const uint32_t lo = __builtin_bit_cast(uint32_t, h01);
            const uint32_t hi = __builtin_bit_cast(uint32_t, h23);
            // split precision: the lo halves fp16(v - hi) (v - hi is exact in fp32)
            const uint32_t llo = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                (float2_t){v[0], v[1]} - __builtin_convertvector(h01, float2_t), half2_t));
            const uint32_t lhi = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                (float2_t){v[2], v[3]} - __builtin_convertvector(h23, float2_t), half2_t));
            for (int d = 0; d < a.ndst; ++d) {
                const int cs = a.dst_cs[d];
                const size_t o = a.dst_coff[d] + ch + prow[i] * cs;
                uint16_t* p = a.dst[d] + o;
                if (vec && ((a.dst_coff[d] | cs) & 3) == 0) {
                    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
                    if constexpr (SPLIT) *reinterpret_cast<uint2*>(a.dst_lo[d] + o) = make_uint2(llo, lhi);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ch + e < a.cout) {
                            p[e] = (uint16_t)((e < 2 ? lo : hi) >> (16 * (e & 1)));
                            if constexpr (SPLIT) a.dst_lo[d][o + e] = (uint16_t)((e < 2 ? llo : lhi) >> (16 * (e & 1)));
                        }
                }
            }
            if (a.out32) {   // fp32 NCHW net output (the activations before fp16)
                int f, yy, xx, sx;
                (void)g.map(pbase + i * 16, f, yy, xx, sx);
                float* o = a.out32 + (((size_t)f * a.out32_c + a.out32_coff + ch) * a.H + yy - g.B) *
                                         a.W + sx * g.sw + xx - g.B;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ch + r < a.cout) o[(size_t)r * a.H * a.W] = v[r];
            }
        }
    }
}

}  // namespace

// Reads: every halo row goes through Strips::map<false>: it maps to a padded-image position of
// [0, frames * (H + 2 B) * (W + 2 B)) (B the net's border, 1 or 3), or -- outside the virtual image
// [0, total) -- to position -1: within the zeroed guards, for either kernel size.  The fragment
// reads stay inside the halo slot: BM + (KS - 1) * (VW + 1) <= HR (conv3_plan checks it).  The
// last strip's columns past the image (nstrips * sw >= W) are masked by Strips::interior.
void launch_conv3s(const ConvArgs& args, const Conv3Plan& p, hipStream_t stream)
{
    OPK_CHECK_ARG(p.family == Conv3Family::conv3s && !args.pool, "conv3s: unsupported conv");
    OPK_CHECK_ARG(p.ks * p.ks == args.ntaps && p.bm + (p.ks - 1) * (p.VW + 1) <= p.hr,
                  "conv3s: strip too wide for the halo");
    OPK_CHECK_ARG(args.in_cs % 8 == 0 && args.in_coff % 8 == 0 && args.in_coff + args.cin_pad <= args.in_cs,
                  "conv3s: input slice unaligned or beyond the buffer");
    bool lo_ok = !args.split || args.in_lo;
    for (int d = 0; d < args.ndst && args.split; ++d) lo_ok = lo_ok && args.dst_lo[d];
    OPK_CHECK_ARG(lo_ok, "conv3s split: lo twins required");
    const ConvArgs a = conv3_planned_args(args, p);
    const dim3 grid((unsigned)p.grid), block(64 * kS_NW);
    bool launched = false;
#define OPK3S_TRY(BM_, BN_, HR_, TAPU_, KS_)                                                   \
    if (!launched && p.bm == BM_ && p.bn == BN_ && p.hr == HR_ && p.tapu == TAPU_ && p.ks == KS_) { \
        note_launch("%s", p.name);                                                             \
        if (a.split)                                                                           \
            hipLaunchKernelGGL((conv3s_kernel<BM_, BN_, HR_, TAPU_, true, KS_>), grid, block, 0, stream, a); \
        else                                                                                   \
            hipLaunchKernelGGL((conv3s_kernel<BM_, BN_, HR_, TAPU_, false, KS_>), grid, block, 0, stream, a); \
        launched = true;                                                                       \
    }
    OPK3S_TRY(64, 32, 256, 9, 3) OPK3S_TRY(128, 64, 320, 3, 3)
    OPK3S_TRY(64, 32, 384, 7, 7) OPK3S_TRY(128, 64, 448, 7, 7)
#undef OPK3S_TRY
    OPK_CHECK_ARG(launched, std::string("no instantiation of ") + p.name);
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
