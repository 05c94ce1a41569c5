// kernels.h -- launchers of the gfx950 kernels in this directory (internal to libopk_hip.so).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace opk {

// ---- resize (resize.hip) -------------------------------------------------------------------
// One source of a resize/merge: [planes][sh][sw] fp32 and its cubic tables on device.
struct ResizeSource {
    const float* src;
    int sh, sw;
    const int* yofs;     // [dh]
    const float* ycoef;  // [dh][4]
    const int* xofs;     // [dw]
    const float* xcoef;  // [dw][4]
    // CUDA-build semantics only (HeatMap::cuda): target pixel x maps to source (x + 0.5) / sx - 0.5
    float sx, sy;
};
constexpr int kMaxResizeSources = 8;
// dst [planes][dh][dw]; planes = frames * channels; all sources share the plane count.
void launch_resize_merge(float* dst, const ResizeSource* srcs, int nsrc, int planes, int dh,
                         int dw, hipStream_t stream);

// A full-resolution heat-map stack [frames][channels][h][w], either materialised in HBM
// (heat != nullptr) or evaluated on the fly, pixel by pixel, as the resize/merge of `nsrc` net
// outputs with exactly the arithmetic of resize.hip (heat_dev.h) -- bit-identical values without
// writing the 75 MB/frame stack.  Consumers: NMS (nms.hip) and PAF scores (paf.hip).
struct HeatMap {
    const float* heat;
    int channels, h, w;
    int nsrc;
    float inv_n;
    ResizeSource src[kMaxResizeSources];
    // 1: the CUDA build's resizeAndMergeGpu arithmetic (heat_dev.h: cuda_bicubic, per-source
    // scale sx / sy, sum / N) instead of cv::resize's; the tables are then unused
    int cuda;
};
// dst [planes][M.h][M.w] = the CUDA-semantics resize/merge (M.cuda) of M's sources
void launch_resize_merge_cuda(float* dst, const HeatMap& M, int planes, hipStream_t stream);
inline HeatMap heat_materialised(const float* heat, int channels, int h, int w)
{
    HeatMap m{};
    m.heat = heat;
    m.channels = channels;
    m.h = h;
    m.w = w;
    return m;
}

// ---- NMS (nms.hip) ----------------------------------------------------------------------------
// peaks [frames][parts][maxPeaks1][3]; heat [frames][channels][h][w].  scratch: nms_scratch_ints()
// ints, zeroed once before the first call (every call leaves it zeroed again).
constexpr int kNmsCandidates = 1024;   // per plane; more peaks fall back to an ordered re-scan
size_t nms_scratch_ints(int frames, int parts);
// cuda: nmsGpu's rules (nmsBase.cu:50-90,161-240: strict interior, 8 strict neighbours, centroid
// sums contracted to fma as nvcc's default --fmad does) instead of nmsCpu's
void launch_nms(float* peaks, int* scratch, const HeatMap& heat, int frames, int parts,
                int max_peaks1, float threshold, float offx, float offy, hipStream_t stream,
                bool cuda = false);

// ---- PAF scores (paf.hip) --------------------------------------------------------------------
struct PafPairTable {
    int npairs;
    int nparts;
    const int* pairs;    // device [2*npairs] (part A, part B)
    const int* mapx;     // device [npairs] heat channel of the x PAF
    const int* mapy;     // device [npairs]
};
// dense: scores [frames][npairs][maxPeaks][maxPeaks]
void launch_paf_scores(float* scores, const HeatMap& heat, const float* peaks, int frames,
                       int max_peaks, const PafPairTable& t, float inter_th,
                       float inter_min_above, float reject_score, double near_dist,
                       hipStream_t stream);
// compact: per frame a record of `rec_floats` floats: [0] = number of scores (or -1 when it did
// not fit), then the nA*nB scores of pair 0, pair 1, ... (row-major i, j).
void launch_paf_scores_compact(float* records, int rec_floats, const HeatMap& heat,
                               const float* peaks, int frames, int max_peaks,
                               const PafPairTable& t, float inter_th, float inter_min_above,
                               float reject_score, double near_dist, hipStream_t stream);
// LDS bytes a workgroup of either launch stages for this map (0: the sources are read directly)
size_t paf_staged_bytes(const HeatMap& heat);

// ---- frames as the callers hand them over (opk_frames of include/opk.h, resolved) ---------------
// n uint8 frames of w x h pixels on the device, packed BGR or YUV 4:2:0.  One description serves
// NV12 and I420: the chroma sample of luma pixel (x, y) of frame f is
// plane[1 | 2][f * frame[1 | 2] + (y >> 1) * cstep + (x >> 1) * cpix].
// B is the byte type of the planes: const where frames are read (FrameSource), writable where
// drawn or converted frames go (FrameDest, opk_frames_out).  A kernel argument: the layout is fixed.
enum FrameFormat { kFramesBgr = 0, kFramesNv12 = 1, kFramesI420 = 2 };
template <class B>
struct FramesT {
    int format;            // FrameFormat
    int n, w, h;
    B* plane[3];           // frame 0 -- BGR: [0]; YUV: Y, U, V (NV12: V = U + 1)
    size_t step, cstep;    // row bytes of plane[0] (BGR or luma) and of the chroma rows
    size_t frame[3];       // bytes from frame f to f + 1 of each plane
    int cpix;              // bytes from one chroma sample to the next: 2 NV12, 1 I420
};
using FrameSource = FramesT<const uint8_t>;
using FrameDest = FramesT<uint8_t>;

// ---- YUV 4:2:0 -> BGR (yuv.hip; the arithmetic: yuv_dev.h) -------------------------------------
// dst BGR uint8 [src.n][src.h][dst_step] (only w*3 bytes of a row are written) from NV12 / I420
void launch_frames_to_bgr(uint8_t* dst, size_t dst_step, const FrameSource& src, hipStream_t stream);
// ---- BGR -> YUV 4:2:0 (yuv.hip; the arithmetic: yuv_out_dev.h) ---------------------------------
// dst NV12 / I420 (only the samples are written) from the BGR frames src of the same n, w, h
void launch_bgr_to_frames(const FrameDest& dst, const FrameSource& src, hipStream_t stream);

// ---- rotated and flipped frames (orient.hip; the definition: include/opk.h) ---------------------
// One plane of a batch as orient.hip's kernels take it: samples of 1, 2 or 3 bytes, the source
// plane w samples x h rows, mx / my the mirror of the source's x / y axis.
struct OrientPlane {
    const uint8_t* src;
    uint8_t* dst;
    size_t sstep, sframe, dstep, dframe;
    int w, h;
    int mx, my;
};
// dst (src's format and n; src.h x src.w pixels when `turn`) = every plane of src permuted:
// D[y][x] = S[sy][sx] with (sx, sy) = (x, y), or (y, x) when `turn`, then mirrored on the source's
// axes by mx / my.  One launch per plane (1 BGR, 2 NV12, 3 I420).
void launch_orient_frames(const FrameDest& dst, const FrameSource& src, bool turn, bool mx, bool my,
                          hipStream_t stream);
// whether launch_orient_frames takes the dword kernels for these frames (else the plain one)
bool orient_tiled(const FrameDest& dst, const FrameSource& src);

// ---- frames to JPEG files (jpeg.hip; the definition: include/opk.h; the arithmetic: jpeg_dev.h) ----
constexpr int kJpegSegMcus = 8;        // consecutive MCUs whose bits one workgroup of jpeg_write assembles
constexpr int kJpegPackBytes = 4096;   // bytes of the bit stream per workgroup of jpeg_count_ff / jpeg_pack
struct JpegTables;
// One chunk of BGR frames through the seven launches of jpeg.hip.  The scratch (host/jpeg_dev.cpp
// lays it out) is per frame of the chunk; the offsets and the destination are the whole batch's.
struct JpegJob {
    const uint8_t* bgr;            // the chunk's first frame
    size_t step, frame;            // row bytes, bytes from frame to frame
    int w, h, frames;              // frames: of this chunk
    int first;                     // index of the chunk's first frame in the batch
    int mcus, segs, pieces;        // per frame: MCUs, ceil(mcus / kJpegSegMcus), rawcap / kJpegPackBytes
    size_t rawcap;                 // bytes of a frame's bit stream scratch: the bound, a multiple of kJpegPackBytes
    const JpegTables* tab;         // device copy
    short* coef;                   // [frames][mcus][6][64] quantised, zigzag order
    unsigned short* blockbits;     // [frames][mcus][6]
    unsigned* segbits;             // [frames][segs]
    unsigned long long* segstart;  // [frames][segs + 1] first bit of each segment; the last: all bits
    uint8_t* raw;                  // [frames][rawcap] the bit stream before stuffing, 16-byte aligned
    unsigned long long* rawbytes;  // [frames] its bytes, the fill included
    unsigned* ffcount;             // [frames][pieces] 0xFF bytes of each piece
    unsigned long long* ffstart;   // [frames][pieces] 0xFF bytes before each piece
    int* fits;                     // [frames] the file ends inside the capacity
    uint8_t* dst;
    size_t capacity;
    unsigned long long* offsets;   // [batch frames + 1]
};
// dwords: every frame base and row step of the chunk is a multiple of 4
void launch_jpeg_chunk(const JpegJob& job, bool dwords, hipStream_t stream);

// ---- frame -> net input (input.hip; YUV sources: yuv.hip) ----------------------------------------
// src: the frames (BGR, or YUV converted on the way: bit for bit the warp of the converted frames);
// dst [n][3][dh][dw] fp32, n output images.
// xtab/ytab: per destination column/row {first source tap, 5-bit fraction index}; wtab: the
// fixed-point 2-D weight table [32*32][ksize*ksize] (host/input.cpp builds all three)
// frame_of (device, may be NULL): source frame of each output image; tab_stride: distance between
// the table pairs of consecutive images, in {tap, fraction} entries (0: one shared pair)
void launch_cvmat_to_input(float* dst, const FrameSource& src, int n, int dh, int dw,
                           const int* xtab, const int* ytab, const short* wtab, int ksize,
                           int normalize, hipStream_t stream, const int* frame_of = nullptr,
                           int tab_stride = 0);
// the YUV routes of launch_cvmat_to_input, which checks the arguments (yuv.hip)
void launch_cvmat_to_input_yuv(float* dst, const FrameSource& src, int n, int dh, int dw,
                               const int* xtab, const int* ytab, const short* wtab, int ksize,
                               int normalize, hipStream_t stream, const int* frame_of,
                               int tab_stride);

// ---- person ids across frames (track.hip; the definition: include/opk.h) ------------------------
// The pyramid of one frame is one record of `frame` bytes: level 0 (the grey image) as uint8
// [h][w] at at[0], level 1 as uint16 (256 x value) at at[1], level 2 as float at at[2]; every level
// starts on a 16-byte boundary of the record.  A batch is n records one after the other.
constexpr int kPyramidLevels = 3;
struct PyramidLayout {
    int levels;
    int w[kPyramidLevels], h[kPyramidLevels];
    size_t at[kPyramidLevels];
    size_t frame;
};
PyramidLayout pyramid_layout(int width, int height, int levels);   // OPK_ERR_ARG: levels not 1..3
// grey + levels 1 .. L.levels - 1 of the frames `src` (BGR, NV12, I420) into pyr [src.n records]
void launch_pyramid(uint8_t* pyr, const PyramidLayout& L, const FrameSource& src, hipStream_t stream);
// dst [n][h][w] fp32 = level `level` of n records
void launch_pyramid_level(float* dst, const uint8_t* pyr, const PyramidLayout& L, int n, int level,
                          hipStream_t stream);
// opk_lk_point: frames frame_i -> frame_j index the records of pyr, -1 the one record `carry`
struct LkPoint {
    int frame_i, frame_j;
    float x, y;
    int status;
};
// every record with status 0 is propagated in place; a frame index outside the buffers (-1 with a
// NULL carry included) gives status 3 and is never followed
void launch_lk_points(LkPoint* points, int npoints, const uint8_t* pyr, int nframes,
                      const uint8_t* carry, const PyramidLayout& L, hipStream_t stream);

// ---- crops of face / hand keypoint extraction (crop.hip) -----------------------------------------
// peaks [crops][parts][3] = (x, y, value) of the maximum of each of the first `parts` channels of
// `heat` (frames = crops), the first in raster order among equal values (cv::minMaxLoc)
void launch_heat_argmax(float* peaks, const HeatMap& heat, int crops, int parts, hipStream_t stream);
// dst[slot[c]][parts][heat.h][heat.w] = ScaleMode-mapped first `parts` channels of crop c (slot -1:
// none), as FaceExtractorCaffe / HandExtractorCaffe store their per-person heat maps
void launch_crop_heatmaps(float* dst, const HeatMap& heat, const int* slot_dev, int crops, int parts,
                          int scale_mode, hipStream_t stream);

// ---- renderers (render.hip) -----------------------------------------------------------------
constexpr int kRenderMaxPeople = 1024;   // people (faces, hands) per frame one launch draws
// One keypoint render (renderKeypointsOld / renderKeypoints, render.hu): frame float BGR [h][w][3]
// in place; kp [people][parts][3]; pairs / colors (RGB) / scales on the device; geom scratch of
// render_geom_floats(people, parts, npairs) floats; eye1 / eye2 the googly-eye parts or -1.
struct RenderKeypointsArgs {
    float* frame;
    int w, h;
    const float* kp;
    int people, parts;
    const unsigned* pairs;
    int npairs;
    const float* colors;
    int ncolors;
    const float* scales;
    int nscales;
    float radius, line_width, threshold, alpha;
    int blend, eye1, eye2;
    float* geom;
};
size_t render_geom_floats(int people, int parts, int npairs);
void launch_render_keypoints(const RenderKeypointsArgs& a, hipStream_t stream);
// the geometry pass alone (a.people may be the people of many frames, frame 0's first: nothing in
// a person's geometry depends on the frame it is drawn on); a.frame is not touched
void launch_render_prep(const RenderKeypointsArgs& a, hipStream_t stream);

// ---- output image: CvMatToOpOutput / OpOutputToCvMat and the fused batch render (render.hip) ----
// The warp of the frames `src` (BGR, or YUV converted on the way) to w x h pixels: ksize 2 / 4
// with the tables of launch_cvmat_to_input, or 0 for the plain copy (then w, h = src.w, src.h)
struct FrameWarp {
    FrameSource src;
    const int* xtab;
    const int* ytab;
    const short* wtab;
    int ksize;
};
// dst float BGR [n][h][w][3]
void launch_cvmat_to_output(float* dst, int n, int w, int h, const FrameWarp& warp,
                            hipStream_t stream);
// dst uint8 [n][h][dst_step] (only w*3 bytes of a row are written) from src float [n][h][w][3];
// cast 0: cvRound + saturate (cv::Mat::convertTo), 1: clamp + truncate (uCharImageCast)
void launch_output_to_cvmat(uint8_t* dst, size_t dst_step, const float* src, int n, int w, int h,
                            int cast, hipStream_t stream);
// One keypoint layer of the fused render: geometry (launch_render_prep's layout over `total`
// people) and the device prefix offsets [n + 1] of each frame's people in it
struct RenderFramesLayer {
    const float* geom;
    const int* offsets;
    int total, parts, npairs;
    const float* colors;
    float alpha;
};
constexpr int kRenderMaxLayers = 3;
// The heat layer of the fused render: what one of the heat-map renders below draws on each frame,
// before the keypoint layers.  `map` is the stack [n][channels][hh][hw] (map.h = hh, map.w = hw),
// materialised (map.heat) or lazy: every value is heat_at(map, f * channels + c, x, y).
enum RenderHeatKind { kHeatNone = 0, kHeatPart, kHeatParts, kHeatPaf, kHeatPafs, kHeatDistance };
struct RenderFramesHeat {
    int kind;
    int channel;           // Part / Distance: the channel; Paf / Pafs: the first x channel
    int count;             // Parts: the parts; Paf: 1; Pafs: the pairs
    float scale, alpha;    // target pixel x samples (x + 0.5) / scale - 0.5
    const float* colors;   // Parts: the RGB table and its rows
    int ncolors;
    int staged;            // set by the launcher: the tile's heat window of this kind fits the LDS
    HeatMap map;
};
// floats of the LDS window a tile's heat values are staged in (the kernel's `items` array)
constexpr int kRenderHeatWindow = 4096;
struct RenderFramesArgs {
    // the drawn frames: BGR, or NV12 / I420 converted from the cast bytes in the store epilogue
    // (yuv_out_dev.h); out.w, out.h, out.n = w, h, n
    FrameDest out;
    int w, h, n;
    FrameWarp warp;
    int blend, cast, nlayers;
    // set by the launcher: every plane base, row step and frame stride of `out` is a multiple of 4
    int dst_aligned;
    // set by the launcher: out.plane[0], out.step and out.frame[0] side by side -- what a BGR store
    // needs in two adjacent scalar loads instead of three scattered ones
    uint8_t* dst;
    size_t dst_step, dst_frame;
    RenderFramesLayer layer[kRenderMaxLayers];
    RenderFramesHeat heat;   // kind kHeatNone: no heat layer
};
// warp -> the heat layer -> every layer in order -> cast, one pass per pixel
void launch_render_frames(const RenderFramesArgs& a, hipStream_t stream);
// whether launch_render_frames stages a tile's heat window of `kind` at `scale` in LDS (else every
// pixel evaluates its own samples)
bool render_heat_staged(int kind, float scale);
// heat-map renders: frame [h][w][3] BGR; heat [channels][hh][hw]; target pixel x samples the heat
// map at (x + 0.5) / scale - 0.5
struct RenderHeatArgs {
    float* frame;
    int w, h;
    const float* heat;
    int hw, hh;
    float scale, alpha;
};
void launch_render_heat_map(const RenderHeatArgs& a, int part, bool abs_value, hipStream_t stream);
void launch_render_heat_maps(const RenderHeatArgs& a, int parts, const float* colors, int ncolors,
                             hipStream_t stream);
void launch_render_pafs(const RenderHeatArgs& a, int first, int count, hipStream_t stream);

// ---- measured ceilings (probe.hip) ------------------------------------------------------------
// operands: 6 x 64 half8 values; out: blocks * 256 floats; 4 waves per workgroup
void launch_mfma_peak(const void* operands, float* out, int blocks, int iters, hipStream_t stream);
void launch_hbm_read(const void* buf, size_t bytes, float* out, int blocks, hipStream_t stream);

// ---- elementwise helpers (misc.hip) -----------------------------------------------------------
void launch_add_inplace(float* dst, const float* src, size_t n, hipStream_t stream);
void launch_delay(int microseconds, hipStream_t stream);   // dev hook: hold a stream
void launch_f64_to_f32(float* dst, const double* src, size_t n, hipStream_t stream);
void launch_f32_to_f64(double* dst, const float* src, size_t n, hipStream_t stream);
// getHeatMapsCopy: dst [frames][nsel][hw] from heat [frames][channels][hw]; sel_dev = nsel source
// channels then nsel kinds (0 part/background, 1 PAF); scale_mode = op::ScaleMode value
void launch_heat_copy(float* dst, const float* heat, const int* sel_dev, int nsel, int frames,
                      int channels, size_t hw, int scale_mode, hipStream_t stream);

// ---- getHeatMapsCopy from the lazy map (heat_out.hip) -----------------------------------------
// The destination channels as up to three runs (parts, background, PAFs): run s = destination
// channels dst0[s] .. dst0[s] + count[s] - 1 from source channels src0[s] .., PAF scaling if paf[s]
struct HeatSelection {
    int nsel;
    int dst0[3], src0[3], count[3], paf[3];
};
// dst [nframes][sel.nsel][M.h][M.w] (float, or uint8 with ScaleMode::UnsignedChar: min(v, 255)) =
// launch_heat_copy of frames frame0 .. of the lazy map M's resize / merge, bit for bit, without
// the materialised stack
void launch_heat_copy_lazy(void* dst, bool u8, const HeatMap& M, const HeatSelection& sel,
                           int frame0, int nframes, int scale_mode, hipStream_t stream);

}  // namespace opk
