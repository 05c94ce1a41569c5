// input.h -- frame -> net input: ScaleAndSizeExtractor + CvMatToOpInput (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../../include/opk.h"
#include "../kernels/kernels.h"
#include "frames.h"

namespace opk {

struct Context;

// op::ScaleAndSizeExtractor::extract (src/openpose/core/scaleAndSizeExtractor.cpp:37-105):
// net input size of every scale (sizes: w, h pairs) and scaleInputToNetInputs.  net_w or net_h
// <= 0 selects the aspect-ratio-derived size (-1x368), bounded by `dyn`
// (--net_resolution_dynamic, > 0) at 16:9.
void scale_and_size(int in_w, int in_h, int net_w, int net_h, float dyn, int scale_number,
                    double scale_gap, double* scales, int* sizes);

// OpenCV's fixed-point tables behind cv::warpAffine on 8-bit images (imgwarp.cpp,
// initInterTab2D): weights [32*32][k*k] (k = 2 linear, 4 cubic; itab zeroed and one entry longer,
// OpenCV's sum correction reads past the last entry), and per destination index of one
// axis {first source tap, fraction index} for the inverse of the diagonal map diag(scale).
void warp_weight_table(bool cubic, short* itab);
void warp_axis_table(double scale, int d, bool cubic, int* tab /* 2*d */);

// (frame_source() / frame_dest(), the checked and resolved descriptors: frames.h)
// the descriptor the pointer-taking entry points fill: n BGR frames [height][step bytes]
inline ::opk_frames bgr_descriptor(const uint8_t* frames, int n, int width, int height, size_t step)
{
    ::opk_frames d{};
    d.format = OPK_FRAMES_BGR;
    d.n = n;
    d.width = width;
    d.height = height;
    d.plane[0] = frames;
    d.step[0] = step;
    return d;
}

// the BGR destination the pointer-taking render entry points describe: n frames [out_h][step bytes]
// (step 0 stays 0 here: render_frames checks it against the row and then takes the tight value)
inline FrameDest bgr_dest(uint8_t* dst, size_t step, int n, int out_w, int out_h)
{
    FrameDest d{};
    d.format = kFramesBgr;
    d.n = n;
    d.w = out_w;
    d.h = out_h;
    d.plane[0] = dst;
    d.step = step;
    return d;
}
// OPK_ERR_ARG when a plane of `dst` shares a byte with another of its planes or frames, or with
// the frames `src` (sample ranges per plane and frame; padding and gaps may interleave)
void check_frames_apart(const FrameDest& dst, const FrameSource& src);
// the destination of a `_to` call on the frames `src`: frame_dest's errors, then a frame count that
// differs from the source's, then check_frames_apart -- all OPK_ERR_ARG before any device work
FrameDest frame_dest_for(const ::opk_frames_out& dst, const FrameSource& src);

// op::CvMatToOpInput::createArray for one scale (cvMatToOpInput.cpp:63-98), a batch of src.n
// frames on device (BGR, or NV12 / I420 converted inside the warp: the values of the BGR path on
// opk_frames_to_bgr's output) -> dst [n][3][dh][dw] fp32 on device
// (resizeFixedAspectRatio + uCharCvMatToFloatPtr with the VGG normalisation when normalize != 0).
// (stream: where the warp runs; nullptr = the context's stream)
void cvmat_to_input(Context* ctx, float* dst, const FrameSource& src, double scale, int dw, int dh,
                    int normalize, hipStream_t stream = nullptr);

}  // namespace opk
