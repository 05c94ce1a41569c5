// context.h -- per-GPU-thread context behind opk_ctx (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../common.h"
#include "../kernels/kernels.h"
#include "pose_model.h"
#include "undistort.h"

struct opk_render_layer;   // include/opk.h
struct opk_render_heat;

namespace opk {

// OpenCV-style cubic tables for one (source size -> target size) axis (host/resize_tables.cpp)
void cubic_tables(int s, int d, int* ofs, float* coef);

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;

    // device copies of cubic tables, keyed by (sh, sw, dh, dw)
    struct Tables { DevBuf buf; const int* yofs; const float* ycoef; const int* xofs; const float* xcoef; };
    std::map<std::tuple<int, int, int, int>, std::unique_ptr<Tables>> resize_tables;
    const Tables& tables(int sh, int sw, int dh, int dw);

    // device pose tables for the PAF kernel
    struct PoseDev { DevBuf buf; PafPairTable t; };
    std::map<int, std::unique_ptr<PoseDev>> pose_dev;
    const PafPairTable& pose_table(int model);

    // frame -> net input (host/input.cpp): fixed-point weight tables (0 linear, 1 cubic) and the
    // per-axis tap tables of each (scale, dw, dh)
    DevBuf warp_weights[2];
    const short* warp_weight_table(bool cubic);
    struct WarpAxes { DevBuf buf; const int* x; const int* y; };
    std::map<std::tuple<uint64_t, int, int>, std::unique_ptr<WarpAxes>> warp_axes;
    const WarpAxes& warp_axis_tables(double scale, int dw, int dh);

    // renderers (host/render.cpp): device copies of the render tables (render_tables.inc) and the
    // per-person geometry scratch of launch_render_keypoints
    struct RenderDev { DevBuf buf; const unsigned* pairs; const float* scales; const float* colors;
                       int npairs, nscales, ncolors; };
    std::map<int, std::unique_ptr<RenderDev>> render_dev;
    const RenderDev& render_table(int which);
    DevBuf render_geom;
    // opk_render_frames (its layers' geometry is in render_geom too): the layers' per-frame
    // prefix offsets on the device and the host copy they were uploaded from (an unchanged batch
    // layout is not uploaded again); the keypoints opk_pose_render_frames uploads
    DevBuf frames_offsets, frames_keypoints;
    std::vector<int> frames_offsets_host;

    DevBuf scratch_scores;   // dense pair scores for opk_connect_body_parts
    // NMS candidate lists (nms.hip), zeroed when (re)allocated; the kernels keep them zeroed
    DevBuf nms_scratch;
    int* nms_candidates(int frames, int parts);
    HostBuf host_peaks, host_scores;
    DevBuf tri_errors;       // opk_triangulate without errors_dev: the points' errors

    // undistortion (host/undistort_dev.cpp): the device maps of every camera set seen, keyed by the
    // parameters' bytes; views with equal parameters share one pair of maps
    struct UndistortDev { DevBuf buf; std::vector<UndistortMap> view; };
    std::map<std::string, std::unique_ptr<UndistortDev>> undistort_maps;
    const UndistortDev& undistort_dev(const UndistortCameras& cams);

    // JPEG frames (host/jpeg_dev.cpp): the device copy of the JpegTables of the last (w, h, quality)
    // seen, the scratch of one chunk of frames, and the BGR frames of a chunk of a YUV source
    DevBuf jpeg_tables, jpeg_scratch, jpeg_bgr;
    int jpeg_key[3] = {0, 0, 0};

    // streams other objects of this context run device work on besides `stream` (PoseHip's
    // post-processing stream, its multi-scale net streams): opk_sync waits for them too
    std::vector<hipStream_t> side_streams;
    void add_side_stream(hipStream_t s) { side_streams.push_back(s); }
    void remove_side_stream(hipStream_t s)
    {
        for (size_t i = 0; i < side_streams.size(); ++i)
            if (side_streams[i] == s) {
                side_streams.erase(side_streams.begin() + (long)i);
                return;
            }
    }

    // device < 0: host-only context (graph planning / host assembly; no device calls)
    void bind() const
    {
        if (device < 0) throw Error(3, "host-only context (device -1) cannot run device work");
        OPK_HIP(hipSetDevice(device));
    }
};

// opk_render_frames (host/render.cpp).  kp_host (may be NULL): layer 0's kp_floats keypoint values
// still on the host (opk_pose_render_frames); they are uploaded after the argument checks.
// heat (may be NULL): the heat layer of opk_render_frames_heat; with `lazy` its values come from
// that map instead of heat->heat_dev (opk_pose_render_frames_element), whose size fields it sets.
// dst: where the drawn frames go, out_w x out_h = dst.w x dst.h -- bgr_dest() of the BGR entry
// points, or a checked opk_frames_out (frame_dest(), host/frames.h) of the `_to` ones.
void render_frames(Context* ctx, const FrameDest& dst, const FrameSource& frames, double scale, const ::opk_render_layer* layers,
                   int n_layers, int blend_original, int cast,
                   const float* kp_host = nullptr, size_t kp_floats = 0,
                   const ::opk_render_heat* heat = nullptr, const HeatMap* lazy = nullptr);
// opk_render_element (host/render.cpp): OPK_HEAT_* kind and channel of a renderPose element
void render_element(int pose_model, int element, int* kind, int* channel);

// Device-time measurement hook (no reference counterpart): while enabled, begin()/end() bracket a
// region of stream work with a pair of HIP events; read() waits for every recorded pair and
// returns their count and summed milliseconds.
class EventTimer {
public:
    ~EventTimer();
    bool on = false;
    void begin(hipStream_t s);
    void end(hipStream_t s);
    void read(int* count, double* total_ms);

private:
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events_, free_;
};

}  // namespace opk
