// render.cpp -- C-ABI (include/opk.h) of the GPU renderers: renderPoseKeypointsGpu and the heat-map
// renders of src/openpose/pose/renderPose.cu:609-866, renderFaceKeypointsGpu
// (src/openpose/face/renderFace.cu:48-76) and renderHandKeypointsGpu
// (src/openpose/hand/renderHand.cu:48-76).  Same argument meaning, launch conditions and error
// texts; the scratch pointers of the reference signatures (maxPtr / minPtr / scalePtr) are not
// needed: the per-person boxes live in the context's own scratch (kernels/render.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/opk.h"
#include "context.h"
#include "input.h"

namespace opk {

namespace {

struct RenderTableRow {
    const char* name;
    const unsigned* pairs;
    int npairs;
    const float* scales;
    int nscales;
    const float* colors;
    int ncolors;
};
#include "render_tables.inc"

enum RenderTable { kRtBody25, kRtCoco, kRtMpi, kRtBody19, kRtBody23, kRtBody25B, kRtBody135,
                   kRtCar12, kRtCar22, kRtFace, kRtHand };

// renderPoseKeypointsGpu's dispatch (renderPose.cu:639-741) and the kernels it launches
// (renderPose.cu:129-417): table, part count, googly-eye parts.  MPI draws MPI pairs / colors with
// COCO_SCALES (renderPose.cu:351) and has no googly eyes.
struct PoseRender {
    int table, scales_table, parts, eye1, eye2;
};
bool pose_render(int model, PoseRender* out)
{
    switch (model) {
    case 0: case 7: case 9: *out = {kRtBody25, kRtBody25, 25, 15, 16}; return true;  // BODY_25/E/D
    case 1: *out = {kRtCoco, kRtCoco, 18, 14, 15}; return true;                       // COCO_18
    case 2: case 3: *out = {kRtMpi, kRtCoco, 15, -1, -1}; return true;                // MPI_15(_4)
    case 4: case 5: case 6: case 12:
        *out = {kRtBody19, kRtBody19, 19, 15, 16}; return true;                       // BODY_19*
    case 8: *out = {kRtCar12, kRtCar12, 12, 4, 5}; return true;                       // CAR_12
    case 10: *out = {kRtBody23, kRtBody23, 23, 13, 14}; return true;                  // BODY_23
    case 11: *out = {kRtCar22, kRtCar22, 22, 6, 7}; return true;                      // CAR_22
    case 13: *out = {kRtBody25B, kRtBody25B, 25, 1, 2}; return true;                  // BODY_25B
    case 14: *out = {kRtBody135, kRtBody135, 135, 1, 2}; return true;                 // BODY_135
    default: return false;
    }
}

void check_alpha(float alpha)
{
    // checkAlpha (renderPose.cu:529-533)
    OPK_CHECK_ARG(!(alpha < 0.f || alpha > 1.f), "Alpha must be in the range [0, 1].");
}

void render_keypoints(Context* ctx, float* frame, unsigned w, unsigned h, const float* kp,
                      int people, int parts, int table, int scales_table, float radius_div,
                      float line_div, float threshold, float alpha, bool blend, int eye1, int eye2)
{
    OPK_CHECK_ARG(people <= kRenderMaxPeople,
                  "at most " + std::to_string(kRenderMaxPeople) + " people per frame");
    OPK_CHECK_ARG(people == 0 || kp != nullptr, "NULL keypoints");
    ctx->bind();
    const auto& t = ctx->render_table(table);
    const auto& st = ctx->render_table(scales_table);
    RenderKeypointsArgs a{};
    a.frame = frame;
    a.w = (int)w;
    a.h = (int)h;
    a.kp = kp;
    a.people = people;
    a.parts = parts;
    a.pairs = t.pairs;
    a.npairs = t.npairs;
    a.colors = t.colors;
    a.ncolors = t.ncolors;
    a.scales = st.scales;
    a.nscales = t.nscales;   // sizeof(<model>_SCALES) even where another table's values are read
    // fastMinCuda(targetWidth, targetHeight) / 100.f etc. (int / float)
    const int m = (int)w < (int)h ? (int)w : (int)h;
    a.radius = (float)m / radius_div;
    a.line_width = (float)m / line_div;
    a.threshold = threshold;
    a.alpha = alpha;
    a.blend = blend ? 1 : 0;
    a.eye1 = eye1;
    a.eye2 = eye2;
    a.geom = static_cast<float*>(
        ctx->render_geom.get(std::max<size_t>(1, render_geom_floats(people, parts, t.npairs)) *
                             sizeof(float)));
    launch_render_keypoints(a, ctx->stream);
}

RenderHeatArgs heat_args(float* frame, unsigned w, unsigned h, const float* heat, int hw, int hh,
                         float scale, float alpha)
{
    OPK_CHECK_ARG(frame && heat, "NULL argument");
    OPK_CHECK_ARG(hw > 0 && hh > 0, "empty heat map");
    check_alpha(alpha);
    return RenderHeatArgs{frame, (int)w, (int)h, heat, hw, hh, scale, alpha};
}

template <class F>
int guarded_render(F&& f)
{
    try {
        f();
        return OPK_OK;
    } catch (const Error& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_error(e.what());
        return OPK_ERR_STATE;
    }
}

}  // namespace

const Context::RenderDev& Context::render_table(int which)
{
    auto it = render_dev.find(which);
    if (it != render_dev.end()) return *it->second;
    const RenderTableRow& r = kRenderTableRows[which];
    const size_t np = 2 * (size_t)r.npairs, nc = 3 * (size_t)r.ncolors;
    std::vector<char> host((np + r.nscales + nc) * 4);
    std::memcpy(host.data(), r.pairs, np * 4);
    std::memcpy(host.data() + np * 4, r.scales, r.nscales * 4);
    std::memcpy(host.data() + (np + r.nscales) * 4, r.colors, nc * 4);
    auto d = std::make_unique<RenderDev>();
    char* dev = static_cast<char*>(d->buf.get(host.size()));
    OPK_HIP(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, stream));
    OPK_HIP(hipStreamSynchronize(stream));
    d->pairs = reinterpret_cast<const unsigned*>(dev);
    d->scales = reinterpret_cast<const float*>(dev + np * 4);
    d->colors = reinterpret_cast<const float*>(dev + (np + r.nscales) * 4);
    d->npairs = r.npairs;
    d->nscales = r.nscales;
    d->ncolors = r.ncolors;
    auto& ref = *d;
    render_dev.emplace(which, std::move(d));
    return ref;
}

namespace {

// ---- the output image (CvMatToOpOutput, OpOutputToCvMat) and the fused batch render -------------

// (the frames' own checks -- format, steps, planes -- are frame_source's, host/frames.h)
void check_output_sizes(int width, int height, int out_w, int out_h, double scale)
{
    // CvMatToOpOutput::createArray's sanity checks (cvMatToOpOutput.cpp:87-90)
    OPK_CHECK_ARG(width > 0 && height > 0, "Input images has 0 area.");
    OPK_CHECK_ARG(out_w > 0 && out_h > 0, "Output resolution has 0 area.");
    OPK_CHECK_ARG(scale > 0 && std::isfinite(scale), "scale must be positive");
}

void check_cast(int cast)
{
    OPK_CHECK_ARG(cast == OPK_CAST_CPU || cast == OPK_CAST_CUDA,
                  "cast: OPK_CAST_CPU (0) or OPK_CAST_CUDA (1)");
}

// resizeFixedAspectRatio (openCvPrivate.cpp:34-53): the copy when nothing changes, else
// cv::warpAffine(diag(scale)) with the tables of the net-input warp (host/input.cpp)
FrameWarp frame_warp(Context* ctx, const FrameSource& src, double scale, int out_w, int out_h)
{
    FrameWarp wp{};
    wp.src = src;
    if (scale != 1. || out_w != src.w || out_h != src.h) {
        const bool cubic = scale > 1.;
        const auto& ax = ctx->warp_axis_tables(scale, out_w, out_h);
        wp.xtab = ax.x;
        wp.ytab = ax.y;
        wp.wtab = ctx->warp_weight_table(cubic);
        wp.ksize = cubic ? 4 : 2;
    }
    return wp;
}

// what renderPoseKeypointsGpu / renderFaceKeypointsGpu / renderHandKeypointsGpu fix for a layer
struct LayerRender {
    int table, scales_table, parts, eye1, eye2, max_people;
    float radius_div, line_div;
};

LayerRender layer_render(const opk_render_layer& l)
{
    check_alpha(l.alpha);
    if (l.kind == OPK_LAYER_FACE) return {kRtFace, kRtFace, 70, -1, -1, kRenderMaxPeople, 120.f, 250.f};
    if (l.kind == OPK_LAYER_HAND) return {kRtHand, kRtHand, 21, -1, -1, kRenderMaxPeople, 100.f, 80.f};
    OPK_CHECK_ARG(l.kind == OPK_LAYER_POSE, "unknown layer kind");
    PoseRender pr{};
    const bool known = pose_render(l.pose_model, &pr);
    OPK_CHECK_ARG(!(l.googly_eyes && (l.pose_model == 2 || l.pose_model == 3)),
                  "Bool googlyEyes not compatible with MPI models.");
    OPK_CHECK_ARG(known, "Invalid Model.");
    return {pr.table, pr.scales_table, pr.parts, l.googly_eyes ? pr.eye1 : -1,
            l.googly_eyes ? pr.eye2 : -1, 127, 100.f, 120.f};
}

// the heat layer's checks (the per-frame heat renders' own, and the stack's bounds) and everything
// of it that needs no device: the kind's channels and the map
RenderFramesHeat heat_layer(const opk_render_heat& h, int n, int blend_original, const HeatMap* lazy)
{
    RenderFramesHeat H{};
    OPK_CHECK_ARG(h.kind >= OPK_HEAT_PART && h.kind <= OPK_HEAT_DISTANCE, "unknown heat kind");
    check_alpha(h.alpha);
    const bool model = h.kind == OPK_HEAT_PARTS || h.kind == OPK_HEAT_PAF || h.kind == OPK_HEAT_PAFS;
    OPK_CHECK_ARG(!model || (h.pose_model >= 0 && h.pose_model < kPoseModels), "Invalid Model.");
    OPK_CHECK_ARG(blend_original != 0,
                  "the heat renders never clear the frame: no blending is alpha 1");
    const int channels = lazy ? lazy->channels : h.channels;
    const int hw = lazy ? lazy->w : h.heat_w, hh = lazy ? lazy->h : h.heat_h;
    OPK_CHECK_ARG(hw > 0 && hh > 0 && channels > 0, "empty heat map");
    static_assert(OPK_HEAT_PART == kHeatPart && OPK_HEAT_PARTS == kHeatParts &&
                      OPK_HEAT_PAF == kHeatPaf && OPK_HEAT_PAFS == kHeatPafs &&
                      OPK_HEAT_DISTANCE == kHeatDistance && OPK_HEAT_NONE == kHeatNone,
                  "OPK_HEAT_* are RenderHeatKind's values");
    H.kind = h.kind;
    H.channel = h.channel;
    H.count = 1;
    int used = 1;
    if (h.kind == OPK_HEAT_PARTS) {
        H.channel = 0;
        H.count = used = pose_model(h.pose_model).parts;
    } else if (h.kind == OPK_HEAT_PAF) {
        used = 2;
    } else if (h.kind == OPK_HEAT_PAFS) {
        // renderPosePAFsGpu (renderPose.cu:818-834): every pair, from the first PAF channel
        const auto& m = pose_model(h.pose_model);
        H.channel = m.parts + (m.bkg ? 1 : 0);
        H.count = m.npairs();
        used = 2 * H.count;
    }
    OPK_CHECK_ARG(H.channel >= 0 && H.channel <= channels - used, "channel outside the heat stack");
    H.scale = h.scale_to_keep_ratio;
    H.alpha = h.alpha;
    if (lazy) {
        H.map = *lazy;
    } else {
        OPK_CHECK_ARG(n == 0 || h.heat_dev, "NULL heat maps");
        H.map = heat_materialised(h.heat_dev, channels, hh, hw);
    }
    return H;
}

}  // namespace

void render_element(int model, int element, int* kind, int* channel)
{
    OPK_CHECK_ARG(model >= 0 && model < kPoseModels, "Invalid Model.");
    const auto& m = pose_model(model);
    // PoseGpuRenderer::renderPose (poseGpuRenderer.cpp:102-202)
    const int parts = m.parts, bkg = m.bkg ? 1 : 0, pb = parts + bkg, pairs = m.npairs();
    const int last_paf = pb + 2 + pairs;
    OPK_CHECK_ARG(element >= 0, "negative element");
    int k = OPK_HEAT_NONE, c = 0;
    if (element == 0) {
    } else if (element == 2) {
        k = OPK_HEAT_PARTS;
    } else if (element == 3) {
        k = OPK_HEAT_PAFS;
        c = pb;
    } else if (element <= pb + 2) {
        k = OPK_HEAT_PART;
        c = element == 1 ? (bkg ? parts : 0) : element - 3 - bkg;
    } else if (element <= last_paf) {
        k = OPK_HEAT_PAF;
        c = pb + m.map_idx.at((size_t)(element - pb - 3) * 2);
    } else {
        OPK_CHECK_ARG(model == 9, "Neck-part distance channel only for BODY_25D.");
        // getNumberElementsToRender (poseParametersRender.cpp:98-113): 2 (parts - 1) of them
        OPK_CHECK_ARG(element <= last_paf + 2 * (parts - 1),
                      "element past the model's last (" +
                          std::to_string(last_paf + 2 * (parts - 1)) + ")");
        k = OPK_HEAT_DISTANCE;
        c = pb + 2 * pairs + (element - last_paf - 1);
    }
    if (kind) *kind = k;
    if (channel) *channel = c;
}

void render_frames(Context* ctx, const FrameDest& dst, const FrameSource& src, double scale,
                   const opk_render_layer* layers, int n_layers, int blend_original, int cast,
                   const float* kp_host, size_t kp_floats, const opk_render_heat* heat,
                   const HeatMap* lazy)
{
    const int n = src.n, out_w = dst.w, out_h = dst.h;
    // everything that does not depend on the frames first, then each frame's counts; device work
    // starts only after the last check
    OPK_CHECK_ARG(n >= 0, "negative frame count");
    OPK_CHECK_ARG(n_layers >= 0 && n_layers <= kRenderMaxLayers, "at most 3 layers");
    OPK_CHECK_ARG(n_layers == 0 || layers, "NULL layers");
    check_cast(cast);
    check_output_sizes(src.w, src.h, out_w, out_h, scale);
    if (dst.format == kFramesBgr)
        OPK_CHECK_ARG(dst.step == 0 || dst.step >= (size_t)out_w * 3, "row step shorter than the row");
    LayerRender lr[kRenderMaxLayers];
    for (int l = 0; l < n_layers; ++l) lr[l] = layer_render(layers[l]);
    RenderFramesHeat heat_args{};
    if (heat) heat_args = heat_layer(*heat, n, blend_original, lazy);
    if (n == 0) return;
    OPK_CHECK_ARG(dst.plane[0] && src.plane[0], "NULL buffer");
    // prefix offsets of every layer: [n_layers][n + 1]
    std::vector<int> offsets((size_t)n_layers * (n + 1));
    size_t geom_floats = 0, geom_at[kRenderMaxLayers] = {};
    for (int l = 0; l < n_layers; ++l) {
        OPK_CHECK_ARG(layers[l].counts_host, "NULL counts");
        int* off = offsets.data() + (size_t)l * (n + 1);
        off[0] = 0;
        for (int f = 0; f < n; ++f) {
            const int c = layers[l].counts_host[f];
            OPK_CHECK_ARG(c >= 0, "negative count");
            if (layers[l].kind == OPK_LAYER_POSE)
                OPK_CHECK_ARG(c <= 127,
                              "Rendering assumes that numberPeople <= POSE_MAX_PEOPLE = 127.");
            OPK_CHECK_ARG(c <= lr[l].max_people,
                          "at most " + std::to_string(kRenderMaxPeople) + " people per frame");
            OPK_CHECK_ARG(off[f] <= (1 << 24) - c, "too many people in the batch");
            off[f + 1] = off[f] + c;
        }
        if (l == 0 && kp_host)
            OPK_CHECK_ARG(kp_floats == (size_t)off[n] * lr[l].parts * 3, "keypoint count");
        else
            OPK_CHECK_ARG(off[n] == 0 || layers[l].keypoints_dev, "NULL keypoints");
        geom_at[l] = geom_floats;
        const auto& row = kRenderTableRows[lr[l].table];
        geom_floats += render_geom_floats(off[n], lr[l].parts, row.npairs);
    }

    ctx->bind();
    RenderFramesArgs a{};
    a.out = dst;
    a.out.n = n;
    if (dst.format == kFramesBgr) {   // the defaults of the pointer-taking form
        if (!a.out.step) a.out.step = (size_t)out_w * 3;
        if (!a.out.frame[0]) a.out.frame[0] = a.out.step * (size_t)out_h;
    }
    a.w = out_w;
    a.h = out_h;
    a.n = n;
    a.warp = frame_warp(ctx, src, scale, out_w, out_h);
    a.blend = blend_original ? 1 : 0;
    a.cast = cast;
    a.nlayers = n_layers;
    a.heat = heat_args;
    if (heat && heat->kind == OPK_HEAT_PARTS) {
        const auto& coco = ctx->render_table(kRtCoco);   // COCO_COLORS (renderPose.cu:427)
        a.heat.colors = coco.colors;
        a.heat.ncolors = coco.ncolors;
    }
    if (n_layers > 0) {
        int* dev = static_cast<int*>(ctx->frames_offsets.get(offsets.size() * sizeof(int)));
        if (offsets != ctx->frames_offsets_host) {
            OPK_HIP(hipMemcpyAsync(dev, offsets.data(), offsets.size() * sizeof(int),
                                   hipMemcpyHostToDevice, ctx->stream));
            OPK_HIP(hipStreamSynchronize(ctx->stream));
            ctx->frames_offsets_host = offsets;
        }
        float* geom = static_cast<float*>(
            ctx->render_geom.get(std::max<size_t>(1, geom_floats) * sizeof(float)));
        const int m = out_w < out_h ? out_w : out_h;
        for (int l = 0; l < n_layers; ++l) {
            const auto& t = ctx->render_table(lr[l].table);
            const auto& st = ctx->render_table(lr[l].scales_table);
            const int total = offsets[(size_t)l * (n + 1) + n];
            // one geometry pass over the layer's people of every frame, with the arguments
            // render_keypoints gives the per-frame renderers
            RenderKeypointsArgs p{};
            p.w = out_w;
            p.h = out_h;
            p.kp = layers[l].keypoints_dev;
            if (l == 0 && kp_host && kp_floats > 0) {
                void* kd = ctx->frames_keypoints.get(kp_floats * sizeof(float));
                OPK_HIP(hipMemcpyAsync(kd, kp_host, kp_floats * sizeof(float),
                                       hipMemcpyHostToDevice, ctx->stream));
                OPK_HIP(hipStreamSynchronize(ctx->stream));
                p.kp = static_cast<const float*>(kd);
            }
            p.people = total;
            p.parts = lr[l].parts;
            p.pairs = t.pairs;
            p.npairs = t.npairs;
            p.colors = t.colors;
            p.ncolors = t.ncolors;
            p.scales = st.scales;
            p.nscales = t.nscales;
            p.radius = (float)m / lr[l].radius_div;
            p.line_width = (float)m / lr[l].line_div;
            p.threshold = layers[l].render_threshold;
            p.alpha = layers[l].alpha;
            p.eye1 = lr[l].eye1;
            p.eye2 = lr[l].eye2;
            p.geom = geom + geom_at[l];
            launch_render_prep(p, ctx->stream);
            a.layer[l] = RenderFramesLayer{p.geom, dev + (size_t)l * (n + 1), total, p.parts,
                                           p.npairs, p.colors, p.alpha};
        }
    }
    launch_render_frames(a, ctx->stream);
}

}  // namespace opk

struct opk_ctx : opk::Context {};

extern "C" {

int opk_render_pose_keypoints(opk_ctx* ctx, float* frame, int pose_model, int people,
                              unsigned width, unsigned height, const float* pose, float threshold,
                              int googly_eyes, int blend_original, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frame, "NULL argument");
        if (!(people > 0 || !blend_original)) return;   // renderPose.cu:616
        opk::PoseRender pr{};
        const bool known = opk::pose_render(pose_model, &pr);
        OPK_CHECK_ARG(!(googly_eyes && (pose_model == 2 || pose_model == 3)),
                      "Bool googlyEyes not compatible with MPI models.");
        OPK_CHECK_ARG(people <= 127,
                      "Rendering assumes that numberPeople <= POSE_MAX_PEOPLE = 127.");
        OPK_CHECK_ARG(known, "Invalid Model.");
        opk::render_keypoints(ctx, frame, width, height, pose, people < 0 ? 0 : people, pr.parts,
                              pr.table, pr.scales_table, 100.f, 120.f, threshold, alpha,
                              blend_original != 0, googly_eyes ? pr.eye1 : -1,
                              googly_eyes ? pr.eye2 : -1);
    });
}

int opk_render_face_keypoints(opk_ctx* ctx, float* frame, unsigned width, unsigned height,
                              const float* face, int people, float threshold, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frame, "NULL argument");
        if (people <= 0) return;   // renderFace.cu:54
        // renderFaceParts (renderFace.cu:21-46): FACE_NUMBER_PARTS 70, radius min/120, line min/250
        opk::render_keypoints(ctx, frame, width, height, face, people, 70, opk::kRtFace,
                              opk::kRtFace, 120.f, 250.f, threshold, alpha, true, -1, -1);
    });
}

int opk_render_hand_keypoints(opk_ctx* ctx, float* frame, unsigned width, unsigned height,
                              const float* hands, int hands_n, float threshold, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frame, "NULL argument");
        if (hands_n <= 0) return;   // renderHand.cu:54
        // renderHandsParts (renderHand.cu:21-46): HAND_NUMBER_PARTS 21, radius min/100, line min/80
        opk::render_keypoints(ctx, frame, width, height, hands, hands_n, 21, opk::kRtHand,
                              opk::kRtHand, 100.f, 80.f, threshold, alpha, true, -1, -1);
    });
}

int opk_render_pose_heat_map(opk_ctx* ctx, float* frame, unsigned width, unsigned height,
                             const float* heat, int heat_w, int heat_h, float scale_to_keep_ratio,
                             unsigned part, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        const auto a = opk::heat_args(frame, width, height, heat, heat_w, heat_h,
                                      scale_to_keep_ratio, alpha);
        ctx->bind();
        opk::launch_render_heat_map(a, (int)part, false, ctx->stream);
    });
}

int opk_render_pose_heat_maps(opk_ctx* ctx, float* frame, int pose_model, unsigned width,
                              unsigned height, const float* heat, int heat_w, int heat_h,
                              float scale_to_keep_ratio, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        const auto a = opk::heat_args(frame, width, height, heat, heat_w, heat_h,
                                      scale_to_keep_ratio, alpha);
        const auto& m = opk::pose_model(pose_model);
        ctx->bind();
        const auto& coco = ctx->render_table(opk::kRtCoco);   // COCO_COLORS (renderPose.cu:427)
        opk::launch_render_heat_maps(a, m.parts, coco.colors, coco.ncolors, ctx->stream);
    });
}

int opk_render_pose_paf(opk_ctx* ctx, float* frame, int pose_model, unsigned width,
                        unsigned height, const float* heat, int heat_w, int heat_h,
                        float scale_to_keep_ratio, int part, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        const auto a = opk::heat_args(frame, width, height, heat, heat_w, heat_h,
                                      scale_to_keep_ratio, alpha);
        (void)opk::pose_model(pose_model);
        ctx->bind();
        opk::launch_render_pafs(a, part, 1, ctx->stream);
    });
}

int opk_render_pose_pafs(opk_ctx* ctx, float* frame, int pose_model, unsigned width,
                         unsigned height, const float* heat, int heat_w, int heat_h,
                         float scale_to_keep_ratio, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        const auto a = opk::heat_args(frame, width, height, heat, heat_w, heat_h,
                                      scale_to_keep_ratio, alpha);
        const auto& m = opk::pose_model(pose_model);
        ctx->bind();
        // renderPosePAFsGpu (renderPose.cu:818-834): every pair, from the first PAF channel
        opk::launch_render_pafs(a, m.parts + (m.bkg ? 1 : 0), m.npairs(), ctx->stream);
    });
}

int opk_render_pose_distance(opk_ctx* ctx, float* frame, unsigned width, unsigned height,
                             const float* heat, int heat_w, int heat_h, float scale_to_keep_ratio,
                             unsigned part, float alpha)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        const auto a = opk::heat_args(frame, width, height, heat, heat_w, heat_h,
                                      scale_to_keep_ratio, alpha);
        ctx->bind();
        // renderPoseDistanceGpu (renderPose.cu:836-864): renderBodyPartHeatMap with absValue
        opk::launch_render_heat_map(a, (int)part, true, ctx->stream);
    });
}

int opk_frames_to_bgr(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, const opk_frames* frames)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frames, "NULL argument");
        const opk::FrameSource src = opk::frame_source(*frames);
        OPK_CHECK_ARG(src.format != OPK_FRAMES_BGR, "BGR frames: nothing to convert");
        OPK_CHECK_ARG(src.w > 0 && src.h > 0, "Input images has 0 area.");
        OPK_CHECK_ARG(dst_step == 0 || dst_step >= (size_t)src.w * 3,
                      "row step shorter than the row");
        if (src.n == 0) return;
        OPK_CHECK_ARG(dst_dev, "NULL buffer");
        ctx->bind();
        opk::launch_frames_to_bgr(dst_dev, dst_step ? dst_step : (size_t)src.w * 3, src,
                                  ctx->stream);
    });
}

int opk_bgr_to_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* bgr_src)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && dst && bgr_src, "NULL argument");
        const opk::FrameSource src = opk::frame_source(*bgr_src);
        OPK_CHECK_ARG(src.format == OPK_FRAMES_BGR, "the source frames must be BGR");
        const opk::FrameDest d = opk::frame_dest_for(*dst, src);
        OPK_CHECK_ARG(d.format != OPK_FRAMES_BGR, "a BGR destination: nothing to convert");
        OPK_CHECK_ARG(src.w > 0 && src.h > 0, "Input images has 0 area.");
        OPK_CHECK_ARG(d.w == src.w && d.h == src.h,
                      "the destination's width and height differ from the source's");
        if (src.n == 0) return;
        OPK_CHECK_ARG(src.plane[0], "NULL buffer");
        ctx->bind();
        opk::launch_bgr_to_frames(d, src, ctx->stream);
    });
}

int opk_render_frames_to(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* frames,
                         double scale_input_to_output, const opk_render_layer* layers, int n_layers,
                         int blend_original, int cast, const opk_render_heat* heat)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && dst && frames, "NULL argument");
        const opk::FrameSource src = opk::frame_source(*frames);
        opk::render_frames(ctx, opk::frame_dest_for(*dst, src), src, scale_input_to_output, layers,
                           n_layers, blend_original, cast, nullptr, 0, heat);
    });
}

int opk_cvmat_to_output_fmt(opk_ctx* ctx, float* output_dev, const opk_frames* frames, double scale,
                            int out_w, int out_h)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frames, "NULL argument");
        const opk::FrameSource src = opk::frame_source(*frames);
        opk::check_output_sizes(src.w, src.h, out_w, out_h, scale);
        if (src.n == 0) return;
        OPK_CHECK_ARG(output_dev && src.plane[0], "NULL buffer");
        ctx->bind();
        opk::launch_cvmat_to_output(output_dev, src.n, out_w, out_h,
                                    opk::frame_warp(ctx, src, scale, out_w, out_h), ctx->stream);
    });
}

int opk_cvmat_to_output(opk_ctx* ctx, float* output_dev, const uint8_t* frames_dev, int n, int width,
                        int height, size_t step, double scale, int out_w, int out_h)
{
    const opk_frames f = opk::bgr_descriptor(frames_dev, n, width, height, step);
    return opk_cvmat_to_output_fmt(ctx, output_dev, &f, scale, out_w, out_h);
}

int opk_output_to_cvmat(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, const float* output_dev,
                        int n, int w, int h, int cast)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx != nullptr, "NULL argument");
        OPK_CHECK_ARG(n >= 0, "negative frame count");
        opk::check_cast(cast);
        OPK_CHECK_ARG(w > 0 && h > 0, "Output resolution has 0 area.");
        OPK_CHECK_ARG(dst_step == 0 || dst_step >= (size_t)w * 3, "row step shorter than the row");
        if (n == 0) return;
        OPK_CHECK_ARG(dst_dev && output_dev, "NULL buffer");
        ctx->bind();
        opk::launch_output_to_cvmat(dst_dev, dst_step ? dst_step : (size_t)w * 3, output_dev, n, w,
                                    h, cast, ctx->stream);
    });
}

int opk_render_frames_heat_fmt(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w,
                               int out_h, const opk_frames* frames, double scale_input_to_output,
                               const opk_render_layer* layers, int n_layers, int blend_original,
                               int cast, const opk_render_heat* heat)
{
    return opk::guarded_render([&] {
        OPK_CHECK_ARG(ctx && frames, "NULL argument");
        const opk::FrameSource src = opk::frame_source(*frames);
        opk::render_frames(ctx, opk::bgr_dest(dst_dev, dst_step, src.n, out_w, out_h), src,
                           scale_input_to_output, layers, n_layers, blend_original, cast, nullptr,
                           0, heat);
    });
}

int opk_render_frames_fmt(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                          const opk_frames* frames, double scale_input_to_output,
                          const opk_render_layer* layers, int n_layers, int blend_original, int cast)
{
    return opk_render_frames_heat_fmt(ctx, dst_dev, dst_step, out_w, out_h, frames,
                                      scale_input_to_output, layers, n_layers, blend_original, cast,
                                      nullptr);
}

int opk_render_frames(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                      const uint8_t* frames_dev, int n, int width, int height, size_t step,
                      double scale_input_to_output, const opk_render_layer* layers, int n_layers,
                      int blend_original, int cast)
{
    const opk_frames f = opk::bgr_descriptor(frames_dev, n, width, height, step);
    return opk_render_frames_heat_fmt(ctx, dst_dev, dst_step, out_w, out_h, &f,
                                      scale_input_to_output, layers, n_layers, blend_original, cast,
                                      nullptr);
}

int opk_render_frames_heat(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                           const uint8_t* frames_dev, int n, int width, int height, size_t step,
                           double scale_input_to_output, const opk_render_layer* layers,
                           int n_layers, int blend_original, int cast, const opk_render_heat* heat)
{
    const opk_frames f = opk::bgr_descriptor(frames_dev, n, width, height, step);
    return opk_render_frames_heat_fmt(ctx, dst_dev, dst_step, out_w, out_h, &f,
                                      scale_input_to_output, layers, n_layers, blend_original, cast,
                                      heat);
}

int opk_render_element(int pose_model, int element, int* kind, int* channel)
{
    return opk::guarded_render([&] { opk::render_element(pose_model, element, kind, channel); });
}

}  // extern "C"
