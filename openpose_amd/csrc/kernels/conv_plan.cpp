// conv_plan.cpp -- which kernel runs a 7x7 / 3x3 / 1x1 conv, on which tile, strips and grid, in
// which frame runs: the one decider behind NetHip's planner (so behind its launch list,
// opk_net_conv_plan and opk_net_conv_kernels) and the probe tools (conv.h).  Plain host
// code: no HIP calls, so the decision is testable without a GPU.
#include "conv.h"

#include <algorithm>
#include <cstdio>

#include "../common.h"
#include "conv_tiles.h"

namespace opk {

namespace {

long ceil_div(long a, long b) { return (a + b - 1) / b; }

int n_block(int cout) { return cout <= 64 ? 64 : (cout <= 96 ? 96 : 128); }

bool want_xhi(const Conv3Query& q) { return q.split && q.xhi && dev_switch("SPLIT_XHI", 1) != 0; }

// the plan's family and tile are on the list of what is instantiated (conv_tiles.h)
void check_instantiated(const Conv3Plan& p)
{
    bool on = false, xhi = false;   // (xhi: the tile has a hi-only instantiation)
    if (p.family == Conv3Family::conv3 || p.family == Conv3Family::conv3s) {
        for (const Conv3Tile& t : kConv3Tiles)
            on = on || (p.bm == t.bm && p.bn == t.bn && p.hr == t.hr && p.tapu == t.tapu && p.minb == t.minb &&
                        p.ks == t.ks && p.nw == t.nw && (p.family == Conv3Family::conv3s) == (t.nw == 4));
        xhi = conv3_tile_has_xhi(p.ks);
    } else if (p.family == Conv3Family::conv3w8) {
        for (const Conv3w8Tile& t : kConv3w8Tiles) on = on || (p.bn == t.bn && p.nb == t.nb && p.pool == t.pool);
        xhi = conv3w8_tile_has_xhi(p.bn, p.pool);
    } else {   // conv3w, conv3p: fp16 only
        for (int bn : kConv3wBNs) on = on || (p.bn == bn && !p.split);
    }
    OPK_CHECK_ARG(on && (!p.xhi || (p.split && xhi)), std::string("no instantiation of ") + p.name);
}

bool aligned(const Conv3Query& q)   // 16-byte stores of 8-channel groups into every destination
{
    bool ok = true;
    for (int d = 0; d < q.ndst; ++d) ok = ok && ((q.dst_coff[d] | q.dst_cs[d]) & 7) == 0;
    return ok;
}

// strips of a row of W columns under a halo of hr rows: BM + (ks - 1) * (VW + 1) rows, VW = sw + 2 B
void strips(Conv3Plan& p, int W, int B)
{
    const int max_strip = (p.hr - p.bm - (p.ks - 1)) / (p.ks - 1) - 2 * B;
    OPK_CHECK_ARG(max_strip >= 8, "conv3: border too wide for the halo");
    p.nstrips = (W + max_strip - 1) / max_strip;
    p.sw = (W + p.nstrips - 1) / p.nstrips;
}

void measure(Conv3Plan& p, const Conv3Query& q, int overhang)
{
    const int B = q.border;
    p.VW = p.sw + 2 * B;
    p.total = (long)q.frames * p.nstrips * (q.H + 2 * B) * p.VW;
    p.fits = conv_positions_fit(p.total + overhang);
    p.grid = ceil_div(p.total, p.bm) * ceil_div(q.cout, p.bn);
    p.workgroups = ceil_div((long)q.frames * q.H * (q.W + 2 * B), p.bm) * ceil_div(q.cout, p.bn);
    p.rcp[0] = (float)(1.0 / ((double)(q.H + 2 * B) * p.VW));
    p.rcp[1] = (float)(1.0 / (double)p.VW);
    p.rcp[2] = (float)(1.0 / (double)p.nstrips);
}

// The tile and strips the conv takes without the small-batch mode.  w8: a 64-output 3x3 conv that
// conv3w8's BN = 64 instantiation can run; persist: the 512 / 688 tile of the persistent kernels
Conv3Plan product_tile(const Conv3Query& q, bool w8, bool& persist)
{
    const int B = q.border;
    Conv3Plan p{};
    p.family = Conv3Family::conv3;
    p.ks = q.ntaps == 49 ? 7 : (q.ntaps == 9 ? 3 : 1);
    p.split = q.split;
    p.bn = p.pbn = n_block(q.cout);
    p.nw = 8;
    persist = false;
    if (p.ks == 1) {   // no halo: small LDS (three tile slots), two workgroups per CU
        p.bm = p.hr = 256;
        p.tapu = 1;
        p.minb = 2;
        p.nstrips = 1;
        p.sw = q.W;
        // dev A/B: CONV1_TILE=1 -> 512x128 tiles of 16 waves, 2 -> 256x256 tiles of 16 waves
        // (cout % 256 == 0): fewer tile rows staged per MFMA than 256x128
        // (default 2: measured -10..-20 % on the 384->512 and 288->256 layers)
        const int t1 = dev_switch("CONV1_TILE", 2);
        if (t1 == 1 && p.bn == 128) {
            p.bm = p.hr = 512; p.nw = 16; p.minb = 1;
        } else if (t1 == 2 && q.cout % 256 == 0) {
            p.bn = p.pbn = 256; p.nw = 16; p.minb = 1;
        } else if (p.bn == 64 && dev_switch("CONV1_N64W16", 0) != 0) {   // dev A/B: 512x64, 16 waves
            p.bm = p.hr = 512; p.nw = 16; p.minb = 1;
        }
        return p;
    }
    if (p.ks == 7) {   // 7x7 (COCO / MPI / face / hand stages): single-tap units, 1024-row halo
        p.bm = 256; p.hr = 1024; p.tapu = 1; p.minb = 1;
    } else {
        // two workgroups per CU pay off once every CU gets at least two 256-position tiles
        // (measured: +10-17 % on the 92x164 / 184x328 / 512-channel layers, -20 % at one tile per
        // CU)
        const long tiles = ((long)q.frames * (q.H + 2 * B) * (q.W + 2 * B) / 256) * ceil_div(q.cout, p.bn);
        // conv3w8 needs strips of more than 16 virtual columns: a narrower 64-output layer is not
        // taken there and keeps conv3_kernel's 8-wave geometry
        if (w8) {
            Conv3Plan n = p;
            n.bm = kConvPersistBM; n.hr = kConvPersistHR;
            strips(n, q.W, B);
            if (n.sw + 2 * B <= 16) w8 = false;
        }
        // (measured, round 1: 4-wave 256x128 two-per-CU tiles and 8-wave 512x128 tiles of 128x64
        // wave tiles were both slower than these on every BODY_25 layer)
        // CONV3_SMALL=0 -> no two-per-CU tiles, CONV3_W16=0 -> no 16-wave tiles,
        // CONV3_PERSIST=0 -> 16-wave tiles without the persistent kernels
        if ((p.bn != 64 || w8) && dev_switch("CONV3_W16", 1) && tiles >= 3 * 256) {
            // 512 x {128, 96} tiles, 16 waves (64 outputs: only for conv3w8's 8 waves of 64 x 64)
            persist = dev_switch("CONV3_PERSIST", 1) != 0;
            p.bm = 512; p.hr = persist ? kConvPersistHR : 704; p.tapu = 3; p.minb = 1; p.nw = 16;
        } else if (dev_switch("CONV3_SMALL", 1) != 0 && tiles >= 2 * 256) {   // <= 80 KB of LDS
            p.bm = 256; p.hr = 448; p.tapu = 1; p.minb = 2;
        } else if (p.bn != 64) {
            p.bm = 256; p.hr = 512; p.tapu = 3; p.minb = 1;
        } else {
            p.bm = 512; p.hr = 768; p.tapu = 3; p.minb = 1;
        }
    }
    strips(p, q.W, B);
    return p;
}

// the plan without the small-batch mode: today's order of tests, every fall-through included
Conv3Plan product_plan(const Conv3Query& q, int only)
{
    const int B = q.border;
    const bool w8 = q.sink && q.cus > 0 && q.cout == 64 && q.ntaps == 9 && q.ndst == 1 && !q.out32 &&
                    aligned(q) && dev_switch("CONV3W8_64", 1) != 0;
    bool persist = false;
    Conv3Plan p = product_tile(q, w8, persist);
    measure(p, q, p.bm + (p.ks - 1) * (p.sw + 2 * B + 1));
    OPK_CHECK_ARG(p.ks == 1 || p.bm + (p.ks - 1) * (p.VW + 1) <= p.hr, "strip too wide for the halo");
    const int nn = (int)ceil_div(q.cout, p.bn);
    // what the persistent kernels need: a sink for masked stores, 16-byte aligned fp16 slices and
    // strips of more than 16 virtual columns
    const bool pers = persist && q.sink && q.cus > 0 && !q.out32 && p.VW > 16 && aligned(q);
    const bool w_ok = pers && (q.cout == 128 || q.cout == 96);
    // conv3w8: 64, 96 or 128 channels, or several 128-channel blocks (the VGG 256 / 512-channel layers)
    const bool w8_ok = pers && q.ndst >= 1 &&
                       (q.cout == 64 || q.cout == 96 || q.cout == 128 || q.cout == 256 || q.cout == 512);
    // its pooled epilogue: windows never straddle a strip or a 6-row tile (even sizes, even
    // strips, 1-pixel border); the pooled image is the one destination
    const bool pool_ok = w8_ok && (q.cout % 128 == 0 || q.cout == 64) && q.ndst == 1 && B == 1 &&
                         q.H % 2 == 0 && q.W % 2 == 0 && p.sw % 2 == 0 && 6 * (p.sw + 2) <= kConvPersistBM;
    Conv3Family f = Conv3Family::conv3;
    if (q.pool && pool_ok) {
        f = Conv3Family::conv3w8;
        p.pool = true;
    } else if (only == (int)Conv3Family::conv3w8 && w8_ok) {
        f = Conv3Family::conv3w8;
    } else if (only == (int)Conv3Family::conv3w && w_ok && !q.split) {
        f = Conv3Family::conv3w;
    } else if (w8 && persist && p.bn == 64) {
        // 64-output layers in the persistent geometry (both precisions): conv3w8's BN = 64 tile
        OPK_CHECK_ARG(w8_ok, "conv3w8<64>: unsupported conv");
        f = Conv3Family::conv3w8;
    } else if (q.split && p.bn != 64 && dev_switch("SPLIT_W8", 1) != 0 && w8_ok) {
        // split precision: every 512-position 96 / 128 / 256 / 512-channel 3x3 layer on conv3w8's
        // split instantiation (bit-identical to conv3_kernel's; SPLIT_W8=0: conv3_kernel, A/B) --
        // its three times longer K loop is the regime where conv3w8 keeps the MFMA pipe busiest;
        // the rest (an fp32 output, unaligned slices, 1x1 heads) on conv3_kernel
        f = Conv3Family::conv3w8;
    } else if (!q.split && nn > 1 && p.bn == 128 && dev_switch("CONV3W8N", 1) != 0 && w8_ok) {
        // several 128-channel n-blocks: conv3w8 with one n-block per persistent block
        // (bit-identical; CONV3W8N=0: the 16-wave conv3_kernel)
        f = Conv3Family::conv3w8;
    } else if (!q.split && nn == 1 && q.cout % p.bn == 0 && pers) {
        // measured: +3-10 % on the single-n-block layers, 3-8 % slower with 2-4 n-blocks (kept 16-wave)
        // mid-unit-barrier schedule (conv3w.hip, bit-identical; CONV3W=0: conv3p_kernel)
        if (dev_switch("CONV3W", 1) != 0 && w_ok) {
            // 8 waves of 64 x 128 (conv3w8.hip, bit-identical): 25 % fewer LDS fragment reads,
            // measured 2-4 % faster from cin 384 up and 4 % slower at cin 128 (tile transitions
            // weigh more there); CONV3W8=0 disables, 2 forces it for 128 outputs, 3 also for 96
            const int s8 = dev_switch("CONV3W8", 1);
            const bool take8 = s8 != 0 && w8_ok &&
                               ((q.cout == 128 && (q.cin_pad >= 384 || s8 >= 2)) || (q.cout == 96 && s8 == 3));
            f = take8 ? Conv3Family::conv3w8 : Conv3Family::conv3w;
        } else {
            f = Conv3Family::conv3p;   // one workgroup per CU
        }
    }
    p.family = f;
    const long ntm = ceil_div(p.total, kConvPersistBM);
    if (f == Conv3Family::conv3w8) {
        p.nw = 8;
        p.nb = q.cout <= 128 ? 1 : q.cout / 128;
        p.bn = p.nb > 1 ? 128 : q.cout;
        // pooled: a tile is six whole virtual rows; a multiple of the n-block count (each block
        // keeps one n-block)
        p.grid = std::min<long>(q.cus / p.nb, p.pool ? (p.total / p.VW - 1 + 5) / 6 : ntm) * p.nb;
        // a split conv over a source without a lo twin: the two-product (XHI) instantiation where
        // the tile has one, logged as conv3w8x_kernel (SPLIT_XHI_W8=0, dev A/B: this family alone
        // on the three-product kernel over a zero twin)
        p.xhi = want_xhi(q) && conv3w8_tile_has_xhi(p.bn, p.pool) && dev_switch("SPLIT_XHI_W8", 1) != 0;
        if (p.xhi)
            std::snprintf(p.name, sizeof p.name, "conv3w8x_kernel<%d,%d", p.bn, p.nb);
        else
            std::snprintf(p.name, sizeof p.name, "conv3w8_kernel<%d,%d,%d", p.bn, p.nb, (int)p.pool);
    } else if (f == Conv3Family::conv3w) {
        p.grid = std::min<long>(q.cus, ntm);
        std::snprintf(p.name, sizeof p.name, "conv3w_kernel<%d", p.bn);
    } else if (f == Conv3Family::conv3p) {
        p.grid = std::min<long>(q.cus, p.grid);
        std::snprintf(p.name, sizeof p.name, "conv3p_kernel<%d", p.bn);
    } else {
        // conv3_kernel's 3x3 instantiations: the 16-wave kernel has 704 halo rows (also over the
        // persistent strip geometry), 64 outputs only 8-wave tiles (512 positions: 768 rows)
        if (p.ks == 3 && p.bn == 64 && p.minb != 2) {
            p.hr = 768; p.nw = 8;
        } else if (p.ks == 3 && p.nw == 16) {
            p.hr = 704;
        }
        // a split conv over a source without a lo twin: the two-product (XHI) instantiation where
        // the tile has one (SPLIT_XHI=0, opk_dev_set, A/B: the three-product kernel over a zero twin)
        p.xhi = want_xhi(q) && conv3_tile_has_xhi(p.ks);
        if (p.nw == 16)
            std::snprintf(p.name, sizeof p.name, "conv3_kernel<%d,%d,%d,%d,1,%d,16%s%s>", p.bm, p.bn, p.hr,
                          p.tapu, p.ks, q.split ? ",split" : "", p.xhi ? ",xhi" : "");
        else
            std::snprintf(p.name, sizeof p.name, "conv3_kernel<%d,%d,%d,%d,%d,%d%s%s>", p.bm, p.bn, p.hr,
                          p.tapu, p.minb, p.ks, q.split ? ",8,split" : "", p.xhi ? ",xhi" : "");
    }
    check_instantiated(p);
    return p;
}

// the conv3s tiles of the conv's kernel size (conv_tiles.h, the smaller first): the larger where
// it gives at least a workgroup per two CUs (7x7: per four, kConv7sBigPerCus) (it stages fewer
// halo and weight bytes and reads fewer LDS fragments per MFMA), else the smaller
bool small_plan(const Conv3Query& q, Conv3Plan& out)
{
    const bool k7 = q.ntaps == 49;
    if (!(k7 ? q.border >= 3 : q.ntaps == 9 && q.border >= 1)) return false;
    bool have = false;
    int seen = 0;
    for (int k = sizeof kConv3Tiles / sizeof kConv3Tiles[0] - 1; k >= 0; --k) {
        const Conv3Tile& tile = kConv3Tiles[k];
        if (tile.nw != 4 || tile.ks != (k7 ? 7 : 3)) continue;
        const bool larger = seen++ == 0;   // (walking the list backwards)
        Conv3Plan s{};
        s.family = Conv3Family::conv3s;
        s.bm = tile.bm; s.bn = tile.bn; s.hr = tile.hr; s.tapu = tile.tapu;
        s.minb = tile.minb; s.ks = tile.ks; s.nw = tile.nw;
        s.split = q.split;
        s.pbn = n_block(q.cout);
        if (s.pbn % s.bn != 0) continue;
        // (a border too wide for the halo: no small tile)
        if ((s.hr - s.bm - (s.ks - 1)) / (s.ks - 1) - 2 * q.border < 8) continue;
        strips(s, q.W, q.border);
        measure(s, q, s.hr);
        if (!s.fits || s.bm + (s.ks - 1) * (s.VW + 1) > s.hr) continue;
        // (the 3x3 names as they were: existing launch logs pin them; 7x7: the kernel size last)
        s.xhi = want_xhi(q) && conv3_tile_has_xhi(s.ks);
        if (k7)
            std::snprintf(s.name, sizeof s.name, "conv3s_kernel<%d,%d,%d,%d,%d%s>", s.bm, s.bn, s.hr,
                          s.tapu, s.ks, q.split ? ",split" : "");
        else
            std::snprintf(s.name, sizeof s.name, "conv3s_kernel<%d,%d,%d,%d%s%s>", s.bm, s.bn, s.hr,
                          s.tapu, q.split ? ",split" : "", s.xhi ? ",xhi" : "");
        out = s;
        have = true;
        // CONV7S_BIG (opk_dev_set, tuning): the larger 7x7 tile from a workgroup per this many CUs
        const int per = k7 ? std::max(1, dev_switch("CONV7S_BIG", kConv7sBigPerCus)) : 2;
        if (larger && per * s.workgroups < std::max(q.cus, 1)) continue;   // (kept if the smaller tile is unsupported)
        break;
    }
    if (have) check_instantiated(out);
    return have;
}

}  // namespace

int conv3_pack_bn(int cout, int ks)
{
    return ks == 1 && dev_switch("CONV1_TILE", 2) == 2 && cout % 256 == 0 ? 256 : n_block(cout);
}

Conv3Query conv3_query(const ConvArgs& a)
{
    Conv3Query q{};
    q.frames = a.frames; q.H = a.H; q.W = a.W;
    q.cout = a.cout; q.cin_pad = a.cin_pad; q.ntaps = a.ntaps; q.border = a.border;
    q.ndst = a.ndst;
    for (int d = 0; d < a.ndst && d < kConvMaxDst; ++d) {
        q.dst_cs[d] = a.dst_cs[d];
        q.dst_coff[d] = a.dst_coff[d];
    }
    q.out32 = a.out32 != nullptr;
    q.split = a.split != 0;
    q.xhi = a.split != 0 && a.in_lo == nullptr;
    q.pool = a.pool != 0;
    q.small = a.small != 0;
    q.sink = a.sink != nullptr;
    q.cus = a.cus;
    return q;
}

Conv3Plan conv3_plan(const Conv3Query& query, int only)
{
    Conv3Query q = query;
    if (q.border <= 0) q.border = 1;
    OPK_CHECK_ARG((q.ntaps == 49 || q.ntaps == 9 || q.ntaps == 1) && q.cin_pad % 32 == 0 && q.cin_pad > 0,
                  "7x7, 3x3 or 1x1, cin_pad % 32 == 0");
    OPK_CHECK_ARG(q.frames > 0 && q.H > 0 && q.W > 0 && q.cout > 0 && q.ndst >= 0 && q.ndst <= kConvMaxDst,
                  "bad sizes");
    OPK_CHECK_ARG(q.border >= (q.ntaps == 49 ? 3 : 1), "conv3: the zero border must cover the pad");
    const Conv3Plan p = product_plan(q, only);
    Conv3Plan s{};
    if (!q.small || p.pool || !small_plan(q, s)) return p;
    // CONV3S_MAX (opk_dev_set, tuning): no small tiles beyond this many workgroups per CU
    const long most = (long)std::max(1, dev_switch("CONV3S_MAX", kConv3sMaxPerCu)) * q.cus;
    if (p.workgroups >= q.cus || s.workgroups <= p.workgroups || s.workgroups > most) return p;
    return s;
}

std::vector<Conv3Run> conv3_runs(const Conv3Query& query)
{
    Conv3Query q = query;
    auto plan = [&](int frames) {
        q.frames = frames;
        return conv3_plan(q);
    };
    const int n = query.frames;
    int run = n;
    for (int runs = 1;; ++runs) {   // the fewest even runs whose every run fits
        run = (n + runs - 1) / runs;
        const int last = n - ((n + run - 1) / run - 1) * run;
        if (plan(run).fits && plan(last).fits) break;
        OPK_CHECK_ARG(run > 1, "one frame exceeds a launch's position range");
    }
    std::vector<Conv3Run> out;
    for (int f0 = 0; f0 < n; f0 += run)
        out.push_back(Conv3Run{f0, std::min(run, n - f0), plan(std::min(run, n - f0))});
    return out;
}

ConvArgs conv3_planned_args(const ConvArgs& a, const Conv3Plan& p)
{
    ConvArgs b = a;
    if (b.border <= 0) b.border = 1;
    OPK_CHECK_ARG(p.fits, "too many positions per launch");
    b.sw = p.sw;
    b.nstrips = p.nstrips;
    for (int i = 0; i < 3; ++i) b.rcp[i] = p.rcp[i];
    if (p.family == Conv3Family::conv3s) b.pbn = p.pbn;
    return b;
}

}  // namespace opk
