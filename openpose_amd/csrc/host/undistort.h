// undistort.h -- undistorted rig frames and the calibration files (include/opk.h): the checked
// camera set, the map of one camera (host), the reader of <serial>.xml, and the device route.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../kernels/kernels.h"

struct opk_cameras;             // include/opk.h
struct opk_camera_parameters;

namespace opk {

struct Context;

struct UndistortCamera {
    double K[9];
    double k[12];   // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, the absent ones 0
    int w, h;
};
struct UndistortCameras {
    std::vector<UndistortCamera> cam;   // empty: none
    int views() const { return (int)cam.size(); }
    std::string key() const;            // the parameters' bytes: what the context caches maps under
};

// the camera set checked as include/opk.h states (OPK_ERR_ARG / OPK_ERR_UNSUPPORTED otherwise)
UndistortCameras make_cameras(const ::opk_cameras* cams);
// OPK_ERR_ARG unless n is a multiple of the views and w x h every view's size
void check_cameras(const UndistortCameras& cams, int n, int w, int h);
// the map of one camera: m1 [h] rows of m1_pitch (x, y) pairs, m2 [h] rows of m2_pitch entries
void undistort_map(const UndistortCamera& c, int16_t* m1, size_t m1_pitch, uint16_t* m2,
                   size_t m2_pitch);
// opk_camera_parameters_read
void camera_parameters_read(const char* dir, const char* const* serials, int n,
                            ::opk_camera_parameters* out, int capacity, int* count);

// ---- the device route (host/undistort_dev.cpp, kernels/undistort.hip) ---------------------------
// One camera's maps on the device, rows padded to a multiple of 4 pixels so that a lane's four
// pixels are one 16-byte and one 8-byte load wherever the row starts.
struct UndistortMap {
    const short2* m1;     // [h][pitch]
    const uint16_t* m2;   // [h][pitch]
    int pitch;
};
// dst (BGR) = the remap of src, frame f with the maps of view f % V, on `stream`; the checks of
// opk_undistort_frames on resolved descriptions (sizes, counts, layout) come first
void undistort_frames(Context* ctx, const FrameDest& dst, const FrameSource& src,
                      const UndistortCameras& cams, hipStream_t stream);
// kernels/undistort.hip: frames first, first + stride, ... of src -> the same frames of dst
void launch_undistort_frames(const FrameDest& dst, const FrameSource& src, const UndistortMap& map,
                             const short* wtab, int first, int stride, hipStream_t stream);

}  // namespace opk
