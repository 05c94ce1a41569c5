// conv3_kernel_body.h -- the body of conv3_kernel and conv3x_kernel (conv3.hip), included inside
// each kernel's braces: the two are the same text, so the instantiations of conv3_kernel compile
// exactly as they did as one function.  Expects the template parameters BM, BN, HR, TAPU, MINB, KS,
// NW and SPLIT in scope, the kernel argument `a`, and OPK3_XHI (false / true) defined.
    constexpr bool XHI = OPK3_XHI;
    static_assert(SPLIT || !XHI, "hi-only source: a split variant");
    constexpr int NP = !SPLIT ? 1 : (XHI ? 2 : 3);   // products per 32-channel input chunk
    constexpr bool SMALL = NW == 4;
    constexpr int WAVES_N = !SMALL && BN % 64 == 0 ? BN / 64 : 2, WAVES_M = NW / WAVES_N;
    constexpr int WROWS = BM / WAVES_M;            // wave tile WROWS x WN
    constexpr int WN = BN / WAVES_N;
    static_assert(WROWS % 16 == 0 && WROWS <= 128 && WN % 16 == 0 && WN <= 64, "wave tiles");
    static_assert(KS == 3 || KS == 7 || (KS == 1 && HR == BM), "3x3, 7x7 or 1x1 (one tap, halo = tile)");
    static_assert((KS * KS) % TAPU == 0, "taps per unit");
    constexpr int MF = WROWS / 16, NF = WN / 16;
    constexpr int KT = KS * KS;                   // taps
    constexpr int UPC = KT / TAPU;                // units per 32-channel chunk
    constexpr int API = HR / 16;                  // halo DMA instructions per block (16 rows each)
    constexpr int AIW = (API + NW - 1) / NW;      // ... per wave, at most
    constexpr int BROWS = TAPU * BN;              // B rows per unit: tap-major, then channel n
    constexpr int BPI = BROWS / 16;               // B DMA instructions per block per unit
    constexpr int BIW = (BPI + NW - 1) / NW;      // ... per wave, at most
    constexpr int ASLOT = HR * 4;                 // 16-byte pieces per halo slot
    constexpr int NAS = UPC >= 2 ? 2 : 3;         // halo slots: unit u+2 may start chunk c+2 if UPC == 1
    constexpr int BSLOT = BROWS * 4;
    constexpr int LDS_PIECES = NAS * ASLOT + 3 * BSLOT;
    static_assert(HR % 16 == 0 && BROWS % 16 == 0, "DMA granularity");
    static_assert(LDS_PIECES * 16 * MINB <= 160 * 1024, "LDS budget");
    static_assert(!SMALL || AIW + BIW <= 15, "vm_wait_rt range");
    __shared__ uint4 lds[LDS_PIECES];

    OPK3_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave - (wave / WAVES_N) * WAVES_N;
    const Strips g(a);
    const int nn = (a.cout + BN - 1) / BN;
    const int tix = tile_order(blockIdx.x, gridDim.x);
    const int p0 = (tix / nn) * BM;
    const int nb = tix - (tix / nn) * nn;
    const int n0 = nb * BN;

    // ---- DMA lane geometry: 16 rows x 4 pieces per wave instruction --------------------------
    const int lrow = lane >> 2, phys = lane & 3;
    const int cpt = a.cin_pad >> 5;               // 32-channel chunks of the input
    // split precision: three products per input chunk c, chunk-major -- virtual chunk 3c + k,
    // k = 0 x_hi w_lo, 1 x_hi w_hi (the hi halo of k = 0 again: no DMA), 2 x_lo w_hi (the lo
    // twin's halo; conv.h OPK_SPLIT_WLO_K); hi halos in slot 0 (UPC == 1: slots 0 / 2 by chunk
    // parity), lo halos in slot 1
    // (XHI: virtual chunk 2c + k, k = 0 x_hi w_lo, 1 x_hi w_hi; hi halos in slots 0 / 1 by
    // chunk parity)
    const int cptk = NP * cpt;                    // K (virtual) chunks
    const int U = UPC * cptk;                     // units (chunk, taps)
    const ptrdiff_t dlo = SPLIT && !XHI ? a.in_lo - a.in : 0;   // hi -> lo twin (elements)
    // halo row hr = (i*NW + wave)*16 + lrow holds virtual position p0 - (KS/2)*(VW + 1) + hr; its
    // image address (chunk 0, swizzled piece) is fixed for the whole tile
    const uint16_t* arow[AIW];
#pragma unroll
    for (int i = 0; i < AIW; ++i) {
        const int hr = (i * NW + wave) * 16 + lrow;
        const int lp = phys ^ (((hr >> 2) & 1) << 1);
        int yy, xx, s;
        int f;
        const long pos = g.template map<false>(p0 - (KS / 2) * (g.VW + 1) + hr, f, yy, xx, s);
        arow[i] = a.in + a.in_coff + pos * a.in_cs + lp * 8;
    }
    // this wave issues halo instructions i*NW + wave < API and B instructions j*NW + wave < BPI
    const int ai = (API - wave + NW - 1) / NW;
    const int bi = (BPI - wave + NW - 1) / NW;
    // the packed n-block (PBN channels, split: w_hi and w_lo, 2 cpt chunks) this tile's BN
    // channels lie in, and their first row in it
    const int pbn = SMALL ? a.pbn : BN;
    const int pb = SMALL ? n0 / pbn : nb, r0 = n0 - pb * pbn;
    const uint16_t* wbase = a.w + (size_t)pb * (SPLIT ? 2 * cpt : cpt) * KT * pbn * 32;
    // weight row rb = (j*NW + wave)*16 + lrow of a unit: tap rb / BN of the unit, channel rb % BN
    int boff[SMALL ? BIW : 1];
    if constexpr (SMALL) {
#pragma unroll
        for (int j = 0; j < BIW; ++j) {
            const int rb = (j * NW + wave) * 16 + lrow;
            boff[j] = ((rb / BN) * pbn + r0 + rb % BN) * 32 + (phys ^ (((rb >> 2) & 1) << 1)) * 8;
        }
    }
    // halo slot of virtual chunk c_ and whether its first unit issues a halo DMA
#define OPK3_ASLOT(c_)                                                                        \
    (!SPLIT ? (c_) % NAS                                                                      \
            : (XHI ? (((c_) / 2) & 1) : ((c_) % 3 == 2 ? 1 : (UPC == 1 ? 2 * (((c_) / 3) & 1) : 0))))
#define OPK3_HALO(c_) (!SPLIT || (XHI ? (c_) % 2 == 0 : (c_) % 3 != 1))
    // packed weight chunk of virtual chunk c_ (split: the cpt w_lo chunks follow the cpt w_hi
    // chunks; the order of conv3w8_kernel, so the two stay bit-identical)
#define OPK3_WCHUNK(c_) ((c_) % NP == OPK_SPLIT_WLO_K ? cpt + (c_) / NP : (c_) / NP)

#define OPK3_ISSUE(u_)                                                                        \
    do {                                                                                      \
        const int c_ = (u_) / UPC, tu_ = (u_) - c_ * UPC;                                     \
        /* dev probe only: 6 = no halo DMA, 7 = no weight DMA after the prologue */           \
        if (tu_ == 0 && OPK3_HALO(c_) && (OPK3_ABLATE != 6 || (u_) < 2)) {                    \
            const int as_ = OPK3_ASLOT(c_) * ASLOT;                                           \
            /* split: k = 2 reads the lo twin, k = 0 the hi image */                          \
            const ptrdiff_t ao_ = !SPLIT ? (ptrdiff_t)c_ * 32                                  \
                                         : (ptrdiff_t)(c_ / NP) * 32 + (!XHI && c_ % 3 == 2 ? dlo : 0); \
            _Pragma("unroll") for (int i_ = 0; i_ < AIW; ++i_)                                \
                if (API % NW == 0 || i_ * NW + wave < API)                                    \
                    __builtin_amdgcn_global_load_lds(                                         \
                        (const void*)(arow[i_] + ao_),                                        \
                        (__attribute__((address_space(3))) void*)(&lds[as_ + (i_ * NW + wave) * 64]), \
                        16, 0, 0);                                                            \
        }                                                                                     \
        const int bs_ = NAS * ASLOT + ((u_) % 3) * BSLOT;                                     \
        /* the unit's weights: TAPU tap blocks of pbn rows (SMALL), else one run of BROWS rows */ \
        const int wc_ = !SPLIT ? c_ : OPK3_WCHUNK(c_);                                        \
        const uint16_t* ub_ =                                                                 \
            SMALL ? wbase + ((size_t)wc_ * KT + tu_ * TAPU) * pbn * 32                        \
                  : wbase + (size_t)(!SPLIT ? (u_) : wc_ * UPC + tu_) * BROWS * 32;           \
        _Pragma("unroll") for (int j_ = 0; j_ < BIW; ++j_) {                                  \
            if ((BPI % NW == 0 || j_ * NW + wave < BPI) && (OPK3_ABLATE != 7 || (u_) < 2)) {  \
                const int rb_ = (j_ * NW + wave) * 16 + lrow;                                 \
                const int lp_ = phys ^ (((rb_ >> 2) & 1) << 1);                               \
                __builtin_amdgcn_global_load_lds(                                             \
                    (const void*)(SMALL ? ub_ + boff[j_] : ub_ + rb_ * 32 + lp_ * 8),         \
                    (__attribute__((address_space(3))) void*)(&lds[bs_ + (j_ * NW + wave) * 64]), \
                    16, 0, 0);                                                                \
            }                                                                                 \
        }                                                                                     \
    } while (0)

    float4_t acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

    const int r16 = lane & 15, q = lane >> 4;
    // bias and negative-side multiplier (1: identity, 0: ReLU, slope: PReLU) of this lane's
    // output channels; fetched before the K loop when registers allow (the older loads retire
    // before the K loop's DMAs: its counted waits cover them)
    float4_t bv[NF], mv[NF];
    const float neg = a.act == 1 ? 0.f : 1.f;
#define OPK3_BIAS()                                                                           \
    do {                                                                                      \
        _Pragma("unroll") for (int j_ = 0; j_ < NF; ++j_) {                                   \
            /* bias/slope arrays are zero-padded to a multiple of 128 channels */             \
            const int ch_ = n0 + wn * WN + j_ * 16 + 4 * q;                                   \
            bv[j_] = *reinterpret_cast<const float4_t*>(a.bias + ch_);                        \
            const float4_t sl_ = *reinterpret_cast<const float4_t*>(a.slope + ch_);           \
            mv[j_] = a.act == 2 ? sl_ : float4_t{neg, neg, neg, neg};                         \
        }                                                                                     \
    } while (0)
    // registers to spare across the K loop
    constexpr bool BIAS_EARLY = SMALL || (MINB == 1 && NW == 8 && MF * NF <= 16);
    if constexpr (BIAS_EARLY) OPK3_BIAS();

    OPK3_ISSUE(0);
    if (U > 1) OPK3_ISSUE(1);
    for (int u = 0; u < U; ++u) {
        const int c = u / UPC, t = u - (u / UPC) * UPC;
        // this wave's loads of unit u have landed once only unit u+1's may still be in flight
        // (unit u+1 carries a halo DMA when it starts a virtual chunk that stages one)
        vm_wait_rt(u + 1 < U ? bi + (t == UPC - 1 && OPK3_HALO(c + 1) ? ai : 0) : 0);
#if OPK3_ABLATE != 3   // dev probe only (3): no block barrier
        __builtin_amdgcn_s_barrier();
#endif
        if (u == 0) OPK3_STAMP(1);
#if OPK3_ABLATE == 2   // dev probe only: no DMA after the prologue (MFMA + LDS-read floor)
        if (u + 2 < U && u + 2 < 3) OPK3_ISSUE(u + 2);
#else
        if (u + 2 < U) OPK3_ISSUE(u + 2);
#endif
        const uint4* As = lds + OPK3_ASLOT(c) * ASLOT;
        const uint4* Bs = lds + NAS * ASLOT + (u % 3) * BSLOT;
#pragma unroll
        for (int k = 0; k < TAPU; ++k) {
            const int tap = t * TAPU + k;         // ky*KS + kx
            const int ky = tap / KS, kx = tap - KS * (tap / KS);
            half8_t fa[MF], fb[NF];
            const int hoff = ky * g.VW + kx;
#if OPK3_ABLATE == 4   // dev probe only: no fragment reads (register operands)
#pragma unroll
            for (int i = 0; i < MF; ++i) fa[i] = (half8_t)(_Float16)(hoff + i);
#pragma unroll
            for (int j = 0; j < NF; ++j) fb[j] = (half8_t)(_Float16)(k + j);
#else
#pragma unroll
            for (int i = 0; i < MF; ++i)
                fa[i] = __builtin_bit_cast(half8_t, As[swz64(wm * WROWS + i * 16 + r16 + hoff, q)]);
#pragma unroll
            for (int j = 0; j < NF; ++j)
                fb[j] = __builtin_bit_cast(half8_t, Bs[swz64(k * BN + wn * WN + j * 16 + r16, q)]);
#endif
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
#if OPK3_ABLATE == 1   // dev probe only: no MFMAs (data movement + sync floor)
                    acc[i][j][0] += (float)fb[j][0] * (float)fa[i][0];
#else
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
#endif
        }
    }
#undef OPK3_ISSUE
#undef OPK3_WCHUNK
#undef OPK3_ASLOT
#undef OPK3_HALO
    OPK3_STAMP(2);
    if constexpr (!BIAS_EARLY) OPK3_BIAS();   // 128-VGPR variants: not kept across the K loop
#undef OPK3_BIAS

    // ---- epilogue straight from registers ------------------------------------------------------
    // lane (q, r16) of fragment (i, j) holds output channels ch..ch+3 (ch = n0 + wn*WN + j*16 + 4q)
    // of virtual position p0 + wm*WROWS + i*16 + r16; border and out-of-image positions are dropped.
    long prow[MF];
    bool pok[MF];
    int pbase = p0 + wm * WROWS + r16;
    asm volatile("" : "+v"(pbase));   // keep the position math after the K loop (register pressure)
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
    // 16-byte stores (see conv3p_kernel): fragment pairs exchanged between lane rows q and q^1 by
    // v_permlane16_swap, each lane then holds 8 consecutive channels of its position.  Needs whole
    // 8-channel groups and 16-byte aligned destination slices; CONV3_WIDE=0 (opk_dev_set) disables.
    bool wide = !SMALL && NF % 2 == 0 && (a.cout & 7) == 0 && !a.out32 && a.wide;
    for (int d = 0; d < a.ndst; ++d) wide = wide && ((a.dst_coff[d] | a.dst_cs[d]) & 7) == 0;
    if (wide) {
        const int cw = n0 + wn * WN + 16 * (q & 1) + 8 * (q >> 1);
#pragma unroll
        for (int j = 0; j + 1 < NF; j += 2) {
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                uint32_t pk[2][2], pl[2][2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    // (split: the sums of the 2^e-scaled weights times 2^-e, exact; conv.h)
                    const float4_t t = (SPLIT ? acc[i][j + h] * a.wscale : acc[i][j + h]) + bv[j + h];
                    const float4_t tm = t * mv[j + h];
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = t[r] > 0.f ? t[r] : tm[r];
                    const half2_t h01 = __builtin_convertvector((float2_t){v[0], v[1]}, half2_t);
                    const half2_t h23 = __builtin_convertvector((float2_t){v[2], v[3]}, half2_t);
                    pk[h][0] = __builtin_bit_cast(uint32_t, h01);
                    pk[h][1] = __builtin_bit_cast(uint32_t, h23);
                    // split precision: lo = fp16(v - hi) (v - hi is exact in fp32)
                    pl[h][0] = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                        (float2_t){v[0], v[1]} - __builtin_convertvector(h01, float2_t), half2_t));
                    pl[h][1] = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                        (float2_t){v[2], v[3]} - __builtin_convertvector(h23, float2_t), half2_t));
                }
                // every lane takes part in the swap; masked lanes store nothing afterwards
                const auto sl = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
                const auto sh = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
                uint4 lval = make_uint4(0, 0, 0, 0);
                if constexpr (SPLIT) {
                    const auto ll = __builtin_amdgcn_permlane16_swap(pl[0][0], pl[1][0], false, false);
                    const auto lh = __builtin_amdgcn_permlane16_swap(pl[0][1], pl[1][1], false, false);
                    lval = make_uint4(ll[0], lh[0], ll[1], lh[1]);
                }
                if (!pok[i] || cw + j * 16 >= a.cout) continue;
                const uint4 val = make_uint4(sl[0], sh[0], sl[1], sh[1]);
                for (int d = 0; d < a.ndst; ++d) {
                    const size_t o = a.dst_coff[d] + cw + j * 16 + prow[i] * a.dst_cs[d];
                    *reinterpret_cast<uint4*>(a.dst[d] + o) = val;
                    if constexpr (SPLIT) *reinterpret_cast<uint4*>(a.dst_lo[d] + o) = lval;
                }
            }
        }
        OPK3_STAMP(5);
        return;
    }
    // fragment column j outer, row i inner: each (i, j) is activated, packed and stored at once
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const float4_t bj = bv[j], mj = mv[j];
        const int ch = chl + j * 16;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            // packed f32 math (v_pk_add/v_pk_mul) and v_cvt_pk_f16_f32 (round to nearest even)
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
            // split precision: the lo halves fp16(v - hi)
            const uint32_t llo = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                (float2_t){v[0], v[1]} - __builtin_convertvector(h01, float2_t), half2_t));
            const uint32_t lhi = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                (float2_t){v[2], v[3]} - __builtin_convertvector(h23, float2_t), half2_t));
            for (int d = 0; d < a.ndst; ++d) {
                const int cs = a.dst_cs[d];
                const size_t o = a.dst_coff[d] + ch + prow[i] * cs;
                uint16_t* p = a.dst[d] + o;
                if (vec && ((a.dst_coff[d] | cs) & 3) == 0) {
#if OPK3_ABLATE == 5   // dev probe only: no output stores
                    asm volatile("" ::"v"(lo), "v"(hi), "v"(p));
#else
                    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
                    if constexpr (SPLIT) *reinterpret_cast<uint2*>(a.dst_lo[d] + o) = make_uint2(llo, lhi);
#endif
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
    OPK3_STAMP(5);
