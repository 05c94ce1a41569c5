// jpeg.hip -- frames to baseline JPEG files on the device (include/opk.h "JPEG FRAMES"; the
// arithmetic: jpeg_dev.h, shared with host/jpeg.cpp; the checks and the chunk walk:
// host/jpeg_dev.cpp).
//
// A chunk of frames goes through seven launches (the frame is grid axis y):
//   jpeg_dct        a wave per MCU: its 16 x 16 pixels come into LDS (as dwords where every base,
//                   step and stride is a multiple of 4 and the MCU lies inside the frame; by bytes
//                   with the edge replication otherwise), a lane converts a 2 x 2 quad, 48 lanes
//                   run a row pass and then a column pass of the six FDCTs, and the quantised
//                   blocks go out in zigzag order as int16 [frame][MCU][6][64].
//   jpeg_count      a wave per block: the non-zero mask of the ACs is one __ballot, a lane's run
//                   comes from the mask, the DC difference from the neighbour's stored DC.  Out:
//                   bits per block and per segment of kJpegSegMcus consecutive MCUs.
//   jpeg_scan_bits  a workgroup per frame: the exclusive scan of the segments' bits.  It also
//                   clears the two dwords of the bit stream that a segment shares with its
//                   neighbours.
//   jpeg_write      a workgroup per segment assembles the segment's bits in LDS at its known
//                   start (an LDS atomicOr per code piece; OR commutes, so the order of arrival
//                   does not matter) and stores whole dwords; only the first and last dword of a
//                   segment can be shared with a neighbour and are ORed into the cleared dword.
//                   The last segment appends the 1-bit fill.
//   jpeg_count_ff   0xFF bytes per kJpegPackBytes of the bit stream.
//   jpeg_scan_ff    a workgroup: the exclusive scan of those counts per frame, the files' sizes,
//                   the packed offsets (carried from chunk to chunk in offsets[] itself) and
//                   whether each file ends inside the capacity.
//   jpeg_pack       a workgroup per kJpegPackBytes: the bytes with a 0x00 after every 0xFF laid out
//                   in LDS, then stored as dwords of the destination (bytes at both ends); the
//                   first one also stores the header, the last one FFD9.  Every store is at an
//                   index below the file's end, which is at most the capacity.
// Nothing depends on arrival order: every value is a pure function of the frames.
#include "kernels.h"
#include "jpeg_dev.h"
#include "../common.h"

namespace opk {

namespace {

constexpr int kWave = 64;
constexpr int kSegBlocks = kJpegSegMcus * 6;
// LDS dwords of a segment's bits: up to 31 bits before its start, its blocks, up to 7 fill bits
constexpr int kSegDwords = (31 + kSegBlocks * kJpegMaxBlockBits + 7 + 31) / 32;

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ int wave_exclusive(int v, int lane)
{
    int incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    return incl - v;
}
// exclusive scan over the 256 threads of a workgroup; *total: the sum.  sh: 8 values of LDS
template <class T>
__device__ __forceinline__ T block_exclusive(T v, T* sh, T* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    __syncthreads();   // sh may still be read from the call before
    if (lane == 63) sh[wv] = incl;
    __syncthreads();
    T before = 0;
    for (int i = 0; i < wv; ++i) before += sh[i];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return before + incl - v;
}

__device__ __forceinline__ void load_huff(JpegHuff* dst, const JpegTables* tab)
{
    const unsigned* s = reinterpret_cast<const unsigned*>(&tab->huff);
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(JpegHuff) / 4); i += blockDim.x) d[i] = s[i];
}

// ---- pass 1: colour, downsample, FDCT, quantisation, zigzag --------------------------------------
// grid (MCUs / 4, frames of the chunk); 4 waves, a wave per MCU
template <bool Dwords>
__global__ __launch_bounds__(256) void jpeg_dct(JpegJob j)
{
    __shared__ unsigned pix[4][16 * 12];    // a wave's 16 rows of 48 bytes
    __shared__ short smp[4][6 * 64];        // samples, then the quantised blocks in natural order
    __shared__ int ws[4][6 * 72];           // row-pass results, rows of 9
    __shared__ unsigned short qv[2 * 64];
    __shared__ unsigned char zz[64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, f = blockIdx.y;
    if (threadIdx.x < 128) qv[threadIdx.x] = j.tab->qv[threadIdx.x >> 6][threadIdx.x & 63];
    if (threadIdx.x < 64) zz[threadIdx.x] = j.tab->zigzag[threadIdx.x];
    const JpegGeom g = jpeg_geom(j.w, j.h);
    const int m_real = blockIdx.x * 4 + wv;
    const int m = m_real < j.mcus ? m_real : j.mcus - 1;   // a wave past the end repeats the last MCU
    const int my = m / g.mw, mx = m - my * g.mw;
    const uint8_t* frame = j.bgr + (size_t)f * j.frame;

    const bool inside = 16 * mx + 16 <= g.w;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int idx = lane + 64 * i, row = idx / 12, dw = idx - row * 12;
        const int y = min(16 * my + row, g.h - 1);
        const uint8_t* src = frame + (size_t)y * j.step;
        unsigned v;
        if (Dwords && inside) {
            v = *reinterpret_cast<const unsigned*>(src + (size_t)mx * 48 + 4 * dw);
        } else {
            v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 4 * dw + e, px = b / 3, c = b - px * 3;
                v |= (unsigned)src[(size_t)jpeg_col(g, 16 * mx + px) * 3 + c] << (8 * e);
            }
        }
        pix[wv][idx] = v;
    }
    __syncthreads();

    {   // a lane per 2 x 2 quad
        const int qy = lane >> 3, qx = lane & 7;
        const int r = 8 * my + qy, c = 8 * mx + qx;
        const uint8_t* p8 = reinterpret_cast<const uint8_t*>(pix[wv]);
        int cb[4], cr[4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ly = 2 * qy + i, lx = 2 * qx + k;
                const uint8_t* p = p8 + ly * 48 + lx * 3;
                int B = p[0], G = p[1], R = p[2];
                smp[wv][(2 * (ly >> 3) + (lx >> 3)) * 64 + (ly & 7) * 8 + (lx & 7)] =
                    (short)jpeg_y(R, G, B);
                if (r >= g.hc) {   // below the last real chroma row: that row's pixels instead
                    const uint8_t* q = frame + (size_t)jpeg_chroma_row(g, r, i) * j.step +
                                       (size_t)jpeg_col(g, 2 * c + k) * 3;
                    B = q[0];
                    G = q[1];
                    R = q[2];
                }
                cb[2 * i + k] = jpeg_cb(R, G, B);
                cr[2 * i + k] = jpeg_cr(R, G, B);
            }
        smp[wv][4 * 64 + lane] = (short)jpeg_downsample(cb[0], cb[1], cb[2], cb[3], c);
        smp[wv][5 * 64 + lane] = (short)jpeg_downsample(cr[0], cr[1], cr[2], cr[3], c);
    }
    __syncthreads();

    const int b = lane >> 3, i8 = lane & 7;   // lanes 0..47: block, and row or column
    if (lane < 48) {
        int d[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) d[x] = smp[wv][b * 64 + i8 * 8 + x] - 128;
        jpeg_fdct_pass<true>(d);
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[wv][b * 72 + i8 * 9 + x] = d[x];
    }
    __syncthreads();
    if (lane < 48) {
        int d[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) d[y] = ws[wv][b * 72 + y * 9 + i8];
        jpeg_fdct_pass<false>(d);
        const unsigned short* q = qv + (b < 4 ? 0 : 64);
#pragma unroll
        for (int y = 0; y < 8; ++y)
            smp[wv][b * 64 + y * 8 + i8] = (short)jpeg_quantise(d[y], q[y * 8 + i8]);
    }
    __syncthreads();

    if (m_real >= j.mcus) return;
    // dummy luma blocks: no ACs, the DC of the block before
    short dc[4];
    dc[0] = smp[wv][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) dc[k] = jpeg_dummy(g, mx, my, k) ? dc[k - 1] : smp[wv][k * 64];
    short* out = j.coef + ((size_t)f * j.mcus + m) * 384;
    const int nat = zz[lane];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        short v = smp[wv][k * 64 + nat];
        if (k > 0 && k < 4 && jpeg_dummy(g, mx, my, k)) v = lane == 0 ? dc[k] : (short)0;
        out[k * 64 + lane] = v;
    }
}

// ---- what a lane puts into the stream for position `lane` of block (m, b) of frame f ---------------
// *eob: the EOB's code, which follows lane 63's own
__device__ __forceinline__ JpegCode lane_code(const JpegJob& j, const JpegHuff& hf, int f, int m,
                                              int b, int lane, JpegCode* eob)
{
    const short* mcu = j.coef + ((size_t)f * j.mcus + m) * 384;
    int v = mcu[b * 64 + lane];
    const uint64_t nz = __ballot(v != 0 && lane > 0);
    if (lane == 0) {
        // the previous block of the component in stream order: luma within the MCU, else the MCU
        // before; 0 at the start of the frame
        int prev = 0;
        if (b > 0 && b < 4) prev = mcu[(b - 1) * 64];
        else if (m > 0) prev = mcu[-384 + (b == 0 ? 3 : b) * 64];
        v -= prev;
    }
    *eob = jpeg_code(hf, b >= 4, 64, 0, nz);
    return jpeg_code(hf, b >= 4, lane, v, nz);
}

// ---- pass 2: bits per block and per segment ----------------------------------------------------------
// grid (segments, frames); a wave per block, blocks wv, wv + 4, ... of the segment
__global__ __launch_bounds__(256) void jpeg_count(JpegJob j)
{
    __shared__ JpegHuff hf;
    __shared__ int part[4];
    load_huff(&hf, j.tab);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, f = blockIdx.y, s = blockIdx.x;
    const int m0 = s * kJpegSegMcus, blocks = min(kJpegSegMcus, j.mcus - m0) * 6;
    int sum = 0;
    for (int i = wv; i < blocks; i += 4) {
        const int m = m0 + i / 6, b = i % 6;
        JpegCode eob;
        const JpegCode c = lane_code(j, hf, f, m, b, lane, &eob);
        const int bits = wave_sum(c.len + (lane == 63 ? eob.len : 0));
        if (lane == 0) j.blockbits[((size_t)f * j.mcus + m) * 6 + b] = (unsigned short)bits;
        sum += bits;
    }
    if (lane == 0) part[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        j.segbits[(size_t)f * j.segs + s] = (unsigned)(part[0] + part[1] + part[2] + part[3]);
}

// ---- pass 3: where every segment starts ---------------------------------------------------------------
// grid (frames)
__global__ __launch_bounds__(256) void jpeg_scan_bits(JpegJob j)
{
    __shared__ unsigned long long sh[8];
    const int f = blockIdx.x;
    const unsigned* bits = j.segbits + (size_t)f * j.segs;
    unsigned long long* start = j.segstart + (size_t)f * (j.segs + 1);
    unsigned* raw = reinterpret_cast<unsigned*>(j.raw + (size_t)f * j.rawcap);
    unsigned long long carry = 0;
    for (int base = 0; base < j.segs; base += 256) {
        const int s = base + (int)threadIdx.x;
        const unsigned long long v = s < j.segs ? bits[s] : 0ull;
        unsigned long long total;
        const unsigned long long at = carry + block_exclusive(v, sh, &total);
        if (s < j.segs) {
            start[s] = at;
            // the dwords this segment may share: its first and its last (the fill included)
            unsigned long long end = at + v;
            if (s == j.segs - 1) end += (0ull - end) & 7ull;
            raw[at >> 5] = 0u;
            raw[(end - 1) >> 5] = 0u;
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        start[j.segs] = carry;
        j.rawbytes[f] = (carry + 7) >> 3;
    }
}

// ---- pass 4: the bit stream ------------------------------------------------------------------------------
__device__ __forceinline__ void lds_put(unsigned* buf, int at, JpegCode c)
{
    int dw = at >> 5, o = at & 31, len = c.len;
    while (len > 0) {
        const int room = 32 - o, take = len < room ? len : room;
        const unsigned piece = (unsigned)((c.bits >> (len - take)) & ((1ull << take) - 1ull));
        atomicOr(&buf[dw], piece << (room - take));
        len -= take;
        ++dw;
        o = 0;
    }
}

// grid (segments, frames)
__global__ __launch_bounds__(256) void jpeg_write(JpegJob j)
{
    __shared__ JpegHuff hf;
    __shared__ unsigned buf[kSegDwords];
    __shared__ int blk_at[kSegBlocks + 1];
    load_huff(&hf, j.tab);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, f = blockIdx.y, s = blockIdx.x;
    const int m0 = s * kJpegSegMcus, blocks = min(kJpegSegMcus, j.mcus - m0) * 6;
    const unsigned long long start = j.segstart[(size_t)f * (j.segs + 1) + s];
    const int lead = (int)(start & 31ull);
    for (int i = threadIdx.x; i < kSegDwords; i += 256) buf[i] = 0u;
    if (wv == 0) {   // where each block starts in buf
        const unsigned short* bb = j.blockbits + ((size_t)f * j.mcus + m0) * 6;
        const int v = lane < blocks ? bb[lane] : 0;
        const int at = wave_exclusive(v, lane);
        if (lane < blocks) blk_at[lane] = lead + at;
        if (lane == blocks - 1) blk_at[blocks] = lead + at + v;
    }
    __syncthreads();
    for (int i = wv; i < blocks; i += 4) {
        const int m = m0 + i / 6, b = i % 6;
        JpegCode eob;
        const JpegCode c = lane_code(j, hf, f, m, b, lane, &eob);
        const int at = blk_at[i] + wave_exclusive(c.len, lane);
        lds_put(buf, at, c);
        if (lane == 63) lds_put(buf, at + c.len, eob);
    }
    int end = blk_at[blocks];
    if (s == j.segs - 1) {   // the frame's last segment: fill the last byte with 1-bits
        const int fill = (int)((0ull - (start + (unsigned long long)(end - lead))) & 7ull);
        if (threadIdx.x == 0 && fill) lds_put(buf, end, JpegCode{(1ull << fill) - 1ull, fill});
        end += fill;
    }
    __syncthreads();
    const int nd = (end + 31) >> 5;
    unsigned* raw = reinterpret_cast<unsigned*>(j.raw + (size_t)f * j.rawcap) + (start >> 5);
    for (int i = threadIdx.x; i < nd; i += 256) {
        const unsigned v = __builtin_bswap32(buf[i]);   // bit 0 of the stream is a byte's MSB
        if (i == 0 || i == nd - 1) atomicOr(&raw[i], v);
        else raw[i] = v;
    }
}

// ---- pass 5: 0xFF bytes per piece of the stream ---------------------------------------------------------
__device__ __forceinline__ int count_ff(uint4 v, int valid)
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    int n = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        n += (i < valid && ((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 0xFFu) ? 1 : 0;
    return n;
}

// grid (pieces, frames); a thread per 16 bytes
__global__ __launch_bounds__(256) void jpeg_count_ff(JpegJob j)
{
    __shared__ int part[4];
    const int f = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bytes = j.rawbytes[f];
    const unsigned long long at = (unsigned long long)blockIdx.x * kJpegPackBytes + 16ull * threadIdx.x;
    int n = 0;
    if (at < bytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(j.raw + (size_t)f * j.rawcap + at);
        n = count_ff(v, (int)min(16ull, bytes - at));
    }
    n = wave_sum(n);
    if (lane == 0) part[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0)
        j.ffcount[(size_t)f * j.pieces + blockIdx.x] = (unsigned)(part[0] + part[1] + part[2] + part[3]);
}

// ---- pass 6: the stuffed pieces' places, the files' sizes and offsets ------------------------------------
// grid (1)
__global__ __launch_bounds__(256) void jpeg_scan_ff(JpegJob j)
{
    __shared__ unsigned long long sh[8];
    if (j.first == 0 && threadIdx.x == 0) j.offsets[0] = 0ull;
    for (int f = 0; f < j.frames; ++f) {
        const unsigned long long bytes = j.rawbytes[f];
        const int used = (int)((bytes + kJpegPackBytes - 1) / kJpegPackBytes);
        unsigned long long carry = 0;
        for (int base = 0; base < used; base += 256) {
            const int p = base + (int)threadIdx.x;
            const unsigned long long v = p < used ? j.ffcount[(size_t)f * j.pieces + p] : 0ull;
            unsigned long long total;
            const unsigned long long at = carry + block_exclusive(v, sh, &total);
            if (p < used) j.ffstart[(size_t)f * j.pieces + p] = at;
            carry += total;
        }
        if (threadIdx.x == 0) {
            const unsigned long long end =
                j.offsets[j.first + f] + kJpegHeaderBytes + bytes + carry + 2ull;
            j.offsets[j.first + f + 1] = end;
            j.fits[f] = end <= (unsigned long long)j.capacity ? 1 : 0;
        }
        __syncthreads();   // offsets[first + f + 1] is the next frame's start
    }
}

// ---- pass 7: the files ------------------------------------------------------------------------------------
// grid (pieces, frames); a thread per 16 bytes of the stream
__global__ __launch_bounds__(256) void jpeg_pack(JpegJob j)
{
    __shared__ int sh[8];
    __shared__ unsigned char out[2 * kJpegPackBytes];
    const int f = blockIdx.y;
    if (!j.fits[f]) return;   // a file that does not fit is not written at all
    const unsigned long long bytes = j.rawbytes[f];
    const unsigned long long piece = (unsigned long long)blockIdx.x * kJpegPackBytes;
    if (piece >= bytes) return;
    const unsigned long long file = j.offsets[j.first + f], file_end = j.offsets[j.first + f + 1];
    uint8_t* dst = j.dst;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < kJpegHeaderBytes; i += 256) dst[file + i] = j.tab->header[i];
    if (piece + kJpegPackBytes >= bytes && threadIdx.x == 0) {
        dst[file_end - 2] = 0xFF;
        dst[file_end - 1] = 0xD9;
    }
    const unsigned long long at = piece + 16ull * threadIdx.x;
    int valid = 0, n = 0;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (at < bytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(j.raw + (size_t)f * j.rawcap + at);
        valid = (int)min(16ull, bytes - at);
        n = count_ff(v, valid);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    int total;
    int pos = 16 * (int)threadIdx.x + block_exclusive(n, sh, &total);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned b = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        if (i < valid) {
            out[pos++] = (unsigned char)b;
            if (b == 0xFFu) out[pos++] = 0;
        }
    }
    __syncthreads();
    // the piece's bytes: dst[lo .. lo + count), stored as the destination's own dwords
    const int count = (int)min((unsigned long long)kJpegPackBytes, bytes - piece) + total;
    const unsigned long long lo =
        file + kJpegHeaderBytes + piece + j.ffstart[(size_t)f * j.pieces + blockIdx.x];
    const int head = (int)((uintptr_t)(dst + lo) & 3u);   // bytes of the first dword before lo
    for (int d = threadIdx.x; 4 * d < head + count; d += 256) {
        const int first = 4 * d - head;   // index into out of the dword's first byte
        if (first >= 0 && first + 4 <= count) {
            const unsigned v = (unsigned)out[first] | (unsigned)out[first + 1] << 8 |
                               (unsigned)out[first + 2] << 16 | (unsigned)out[first + 3] << 24;
            *reinterpret_cast<unsigned*>(dst + lo + first) = v;
        } else {
            for (int e = 0; e < 4; ++e)
                if (first + e >= 0 && first + e < count) dst[lo + first + e] = out[first + e];
        }
    }
}

}  // namespace

void launch_jpeg_chunk(const JpegJob& j, bool dwords, hipStream_t stream)
{
    OPK_CHECK_ARG(j.frames > 0 && j.frames <= 65535 && j.mcus > 0 && j.segs > 0 && j.pieces > 0,
                  "empty chunk");
    OPK_CHECK_ARG(j.rawcap % kJpegPackBytes == 0 &&
                      j.rawcap >= ((size_t)j.mcus * 6 * kJpegMaxBlockBits + 7) / 8 + 4,
                  "bit stream scratch smaller than the bound");
    const dim3 tb(256);
    const unsigned fr = (unsigned)j.frames;
    // dev switch JPEG_PASSES (tools/jpeg_bench.py): stop after that many launches, so that the
    // differences of the totals are the passes' times; unset: all seven
    const int passes = dev_switch("JPEG_PASSES", 7);
    note_launch("jpeg_dct<%s>", dwords ? "dwords" : "bytes");
    if (dwords) hipLaunchKernelGGL(jpeg_dct<true>, dim3((unsigned)((j.mcus + 3) / 4), fr), tb, 0, stream, j);
    else hipLaunchKernelGGL(jpeg_dct<false>, dim3((unsigned)((j.mcus + 3) / 4), fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 2) return;
    note_launch("jpeg_count");
    hipLaunchKernelGGL(jpeg_count, dim3((unsigned)j.segs, fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 3) return;
    note_launch("jpeg_scan_bits");
    hipLaunchKernelGGL(jpeg_scan_bits, dim3(fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 4) return;
    note_launch("jpeg_write");
    hipLaunchKernelGGL(jpeg_write, dim3((unsigned)j.segs, fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 5) return;
    note_launch("jpeg_count_ff");
    hipLaunchKernelGGL(jpeg_count_ff, dim3((unsigned)j.pieces, fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 6) return;
    note_launch("jpeg_scan_ff");
    hipLaunchKernelGGL(jpeg_scan_ff, dim3(1), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
    if (passes < 7) return;
    note_launch("jpeg_pack");
    hipLaunchKernelGGL(jpeg_pack, dim3((unsigned)j.pieces, fr), tb, 0, stream, j);
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
