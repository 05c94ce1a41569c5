// api_net.cpp -- C-ABI (include/opk.h): NetHip (op::NetCaffe) and PoseHip
// (op::PoseExtractorCaffe) entry points.
#include <cstring>
#include <memory>
#include <string>

#include "../../../include/opk.h"
#include "net.h"
#include "caffemodel.h"
#include "extract.h"
#include "input.h"
#include "pose.h"
#include "track.h"

namespace opk {
template <class F>
static int guarded_net(F&& f)
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
}  // namespace opk

struct opk_ctx : opk::Context {};
struct opk_net {
    opk_ctx* ctx;
    std::unique_ptr<opk::NetHip> net;
};
struct opk_pose {
    opk_ctx* ctx;
    std::unique_ptr<opk::PoseHip> pose;
};

using opk::guarded_net;

extern "C" {

int opk_net_create(opk_ctx* ctx, const char* prototxt, const char* caffemodel, opk_net** out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx && prototxt && out, "NULL argument");
        const std::string p(prototxt);
        std::vector<opk::LayerDesc> layers =
            p.rfind("builtin:", 0) == 0 ? opk::builtin_graph(p) : opk::load_prototxt(p);
        auto n = std::make_unique<opk_net>(opk_net{ctx, std::make_unique<opk::NetHip>(ctx, std::move(layers))});
        if (caffemodel && caffemodel[0]) {
            OPK_CHECK_ARG(ctx->device >= 0, "weights need a device context");
            n->net->load_caffemodel(caffemodel);
        }
        *out = n.release();
    });
}

int opk_net_destroy(opk_net* net)
{
    return guarded_net([&] {
        if (!net) return;
        if (net->ctx->device >= 0) net->ctx->bind();
        delete net;
    });
}

int opk_net_num_convs(opk_net* net)
{
    if (!net) return -1;
    return (int)net->net->convs().size();
}

int opk_net_conv_info(opk_net* net, int i, char* name, int* cin, int* cout, int* k, int* act)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && i >= 0 && i < (int)net->net->convs().size(), "bad index");
        const auto& c = net->net->convs()[i];
        if (name) {
            std::strncpy(name, c.name.c_str(), 63);
            name[63] = 0;
        }
        if (cin) *cin = c.cin;
        if (cout) *cout = c.cout;
        if (k) *k = c.k;
        if (act) *act = c.act;
    });
}

int opk_net_set_conv(opk_net* net, const char* name, const float* w, const float* b,
                     const float* slope)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && name, "NULL argument");
        net->net->set_conv(name, w, b, slope);
    });
}

int opk_net_forward(opk_net* net, const float* input, int n, int h, int w)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->forward(input, n, h, w);
    });
}

int opk_net_flops_per_frame(opk_net* net, int h, int w, double* flops)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && flops && h > 0 && w > 0, "bad argument");
        *flops = net->net->flops_per_frame(h, w);
    });
}

int opk_net_output(opk_net* net, float** out, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && out && shape, "NULL argument");
        *out = net->net->output();   // NULL (and a {0, C, 0, 0} shape) before the first forward
        shape[0] = net->net->frames();
        shape[1] = net->net->out_channels();
        shape[2] = net->net->out_h();
        shape[3] = net->net->out_w();
    });
}

int opk_net_blob(opk_net* net, const char* name, int frame0, int nframes, float* host_out,
                 int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && name && shape, "NULL argument");
        net->net->blob(name, frame0, nframes, host_out, shape);
    });
}

int opk_net_blob_planes(opk_net* net, const char* name, int frame0, int nframes, float* hi_host,
                        float* lo_host, int shape[4], int* has_lo)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && name && shape && has_lo, "NULL argument");
        net->net->blob_planes(name, frame0, nframes, hi_host, lo_host, shape, has_lo);
    });
}

int opk_net_launch_log(opk_net* net, char* buf, size_t size, size_t* needed)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && needed, "NULL argument");
        std::string text;
        for (const auto& l : net->net->launches()) text += l + "\n";
        *needed = text.size() + 1;
        if (buf && size >= *needed) std::memcpy(buf, text.c_str(), text.size() + 1);
    });
}

int opk_pose_create(opk_ctx* ctx, opk_net* net, int maxpos, opk_pose** out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx && out, "NULL argument");
        *out = new opk_pose{ctx, std::make_unique<opk::PoseHip>(ctx, net ? net->net.get() : nullptr,
                                                                maxpos != 0)};
    });
}

int opk_pose_create_model(opk_ctx* ctx, opk_net* net, int pose_model, int maxpos, int semantics,
                          opk_pose** out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx && out, "NULL argument");
        *out = new opk_pose{ctx, std::make_unique<opk::PoseHip>(ctx, net ? net->net.get() : nullptr,
                                                                maxpos != 0, pose_model, semantics)};
    });
}

int opk_pose_destroy(opk_pose* p)
{
    return guarded_net([&] {
        if (!p) return;
        if (p->ctx->device >= 0) p->ctx->bind();
        delete p;
    });
}

int opk_pose_set_map_semantics(opk_pose* p, int semantics)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_map_semantics(semantics);
    });
}

int opk_pose_set_property(opk_pose* p, int prop, double v)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_property(prop, v);
    });
}

int opk_pose_forward(opk_pose* p, const float* frames, int n, int net_h, int net_w, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->forward(frames, n, net_h, net_w, pw, ph);
    });
}

int opk_pose_forward_net_output(opk_pose* p, const float* out, int n, int oh, int ow, int net_h,
                                int net_w, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->forward_net_output(out, n, oh, ow, net_h, net_w, pw, ph);
    });
}

int opk_pose_submit(opk_pose* p, const float* frames, int n, int net_h, int net_w, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->submit(frames, n, net_h, net_w, pw, ph);
    });
}

int opk_pose_submit_multi(opk_pose* p, const float* const* frames, const int* net_hw, int nscales,
                          int n, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->submit_multi(frames, net_hw, nscales, n, pw, ph);
    });
}

int opk_pose_forward_multi(opk_pose* p, const float* const* frames, const int* net_hw,
                           int nscales, int n, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(p->pose->pending() == 0, "batches in flight: collect them first");
        p->pose->submit_multi(frames, net_hw, nscales, n, pw, ph);
        p->pose->collect();
    });
}

int opk_pose_submit_net_output(opk_pose* p, const float* out, int n, int oh, int ow, int net_h,
                               int net_w, int pw, int ph)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->submit_net_output(out, n, oh, ow, net_h, net_w, pw, ph);
    });
}

int opk_pose_collect(opk_pose* p, int* frames)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        const int n = p->pose->collect();
        if (frames) *frames = n;
    });
}

int opk_pose_pending(opk_pose* p) { return p ? p->pose->pending() : -1; }

int opk_pose_set_upsampling_ratio(opk_pose* p, float ratio)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_upsampling_ratio(ratio);
    });
}

int opk_pose_set_overlay(opk_pose* p, const float* overlay)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_overlay(overlay);
    });
}

int opk_pose_num_people(opk_pose* p, int frame)
{
    if (!p || frame < 0 || frame >= p->pose->frames()) return -1;
    return p->pose->num_people(frame);
}

int opk_pose_keypoints(opk_pose* p, int frame, float* kp, float* ks, int max_people)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && frame >= 0 && frame < p->pose->frames(), "bad frame");
        const int n = std::min(max_people, p->pose->num_people(frame));
        const auto& k = p->pose->keypoints(frame);
        const auto& s = p->pose->scores(frame);
        const int parts = opk::pose_model(p->pose->model()).parts;
        if (kp && n > 0) std::memcpy(kp, k.data(), sizeof(float) * n * parts * 3);
        if (ks && n > 0) std::memcpy(ks, s.data(), sizeof(float) * n);
    });
}

int opk_pose_set_timing(opk_pose* p, int enable)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_timing(enable != 0);
    });
}

int opk_pose_read_timing(opk_pose* p, int* batches, double* total_ms)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->read_timing(batches, total_ms);
    });
}

int opk_pose_read_collect_times(opk_pose* p, int* collects, double* wait_ms, double* assembly_ms,
                                int* workers)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->read_collect_times(collects, wait_ms, assembly_ms);
        if (workers) *workers = p->pose->assembly_workers();
    });
}

int opk_pose_records(opk_pose* p, float* rec, size_t capacity, size_t* used)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && used, "NULL argument");
        const opk::PoseHip& pose = *p->pose;
        const int parts = opk::pose_model(pose.model()).parts;
        size_t need = 0;
        for (int f = 0; f < pose.frames(); ++f) need += 1 + (size_t)pose.num_people(f) * (parts * 3 + 1);
        *used = need;
        if (!rec) return;
        OPK_CHECK_ARG(capacity >= need, "records buffer too small");
        float* o = rec;
        for (int f = 0; f < pose.frames(); ++f) {
            const int n = pose.num_people(f);
            *o++ = (float)n;
            if (n == 0) continue;
            std::memcpy(o, pose.keypoints(f).data(), sizeof(float) * n * parts * 3);
            o += (size_t)n * parts * 3;
            std::memcpy(o, pose.scores(f).data(), sizeof(float) * n);
            o += n;
        }
    });
}

int opk_pose_heatmaps(opk_pose* p, float** heat, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && heat && shape, "NULL argument");
        *heat = p->pose->heatmaps(shape);
    });
}

int opk_pose_heatmap_size(opk_pose* p, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && shape, "NULL argument");
        p->pose->heatmap_size(shape);
    });
}

int opk_pose_peaks(opk_pose* p, float** peaks, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && peaks && shape, "NULL argument");
        *peaks = p->pose->peaks(shape);
    });
}

int opk_net_load_caffemodel(opk_net* net, const char* caffemodel, int* loaded)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && caffemodel, "NULL argument");
        OPK_CHECK_ARG(net->ctx->device >= 0, "weights need a device context");
        const int n = net->net->load_caffemodel(caffemodel);
        if (loaded) *loaded = n;
    });
}

int opk_caffemodel_blob(const char* caffemodel, const char* layer, int index, float* data,
                        size_t capacity, int64_t* shape, int* ndim)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(caffemodel && layer && ndim, "NULL argument");
        const auto layers = opk::load_caffemodel(caffemodel);
        for (const auto& L : layers) {
            if (L.name != layer) continue;
            OPK_CHECK_ARG(index >= 0 && index < (int)L.blobs.size(), "no such blob");
            const auto& b = L.blobs[index];
            OPK_CHECK_ARG(b.shape.size() <= 8, "blob rank > 8");
            *ndim = (int)b.shape.size();
            if (shape) for (size_t i = 0; i < b.shape.size(); ++i) shape[i] = b.shape[i];
            if (data) {
                OPK_CHECK_ARG(capacity >= b.data.size(), "capacity too small");
                std::memcpy(data, b.data.data(), b.data.size() * sizeof(float));
            }
            return;
        }
        throw opk::Error(1, std::string("layer ") + layer + " has no blobs in " + caffemodel);
    });
}

int opk_net_set_precision(opk_net* net, int precision)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->set_precision(precision);
    });
}

int opk_net_set_precision_schedule(opk_net* net, const int* precisions, int count)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->set_precision_schedule(precisions, count);
    });
}

int opk_net_conv_precision(opk_net* net, int index)
{
    if (!net) return -1;
    return net->net->conv_precision(index);
}

int opk_net_set_small_batch(opk_net* net, int enable)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        OPK_CHECK_ARG(enable == 0 || enable == 1, "small batch: 0 or 1");
        net->net->set_small_batch(enable == 1);
    });
}

int opk_net_small_batch(opk_net* net)
{
    if (!net) return -1;
    return net->net->small_batch() ? 1 : 0;
}

int opk_net_conv_plan(opk_net* net, int index, int n, int h, int w, int cus, int* bm, int* bn,
                      int* workgroups, int* small)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->conv_plan(index, n, h, w, cus, bm, bn, workgroups, small);
    });
}

int opk_net_conv_kernels(opk_net* net, int index, int n, int h, int w, int cus, char* buf, size_t size,
                         size_t* needed)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net && needed, "NULL argument");
        std::string text;
        for (const auto& k : net->net->conv_kernels(index, n, h, w, cus)) text += k + "\n";
        *needed = text.size() + 1;
        if (buf && size >= *needed) std::memcpy(buf, text.c_str(), text.size() + 1);
    });
}

int opk_net_set_timing(opk_net* net, int enable)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->set_timing(enable != 0);
    });
}

int opk_net_read_timing(opk_net* net, int* forwards, double* total_ms)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(net, "NULL net");
        net->net->read_timing(forwards, total_ms);
    });
}

int opk_scale_and_size(int in_w, int in_h, int net_w, int net_h, float dynamic_behavior,
                       int scale_number, double scale_gap, double* scales, int* net_sizes)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(scales && net_sizes, "NULL output");
        opk::scale_and_size(in_w, in_h, net_w, net_h, dynamic_behavior, scale_number, scale_gap,
                            scales, net_sizes);
    });
}

int opk_cvmat_to_input_fmt(opk_ctx* ctx, float* input_dev, const opk_frames* frames, double scale,
                           int net_w, int net_h, int normalize)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx, "NULL context");
        OPK_CHECK_ARG(frames, "NULL frames");
        OPK_CHECK_ARG(normalize == 0 || normalize == 1,
                      "normalize: 0 (none) or 1 (VGG); DenseNet (2) is not supported");
        opk::cvmat_to_input(ctx, input_dev, opk::frame_source(*frames), scale, net_w, net_h,
                            normalize);
    });
}

int opk_cvmat_to_input(opk_ctx* ctx, float* input_dev, const uint8_t* frames_dev, int n, int width,
                       int height, size_t step, double scale, int net_w, int net_h, int normalize)
{
    const opk_frames f = opk::bgr_descriptor(frames_dev, n, width, height, step);
    return opk_cvmat_to_input_fmt(ctx, input_dev, &f, scale, net_w, net_h, normalize);
}

int opk_pose_set_input(opk_pose* p, int net_w, int net_h, float dynamic_behavior, int scale_number,
                       double scale_gap)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_input(net_w, net_h, dynamic_behavior, scale_number, scale_gap);
    });
}

int opk_pose_submit_frames_fmt(opk_pose* p, const opk_frames* frames)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        p->pose->submit_frames(opk::frame_source(*frames));
    });
}

int opk_pose_forward_frames_fmt(opk_pose* p, const opk_frames* frames)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        p->pose->forward_frames(opk::frame_source(*frames));
    });
}

int opk_pose_submit_frames(opk_pose* p, const uint8_t* frames, int n, int width, int height,
                           size_t step)
{
    const opk_frames f = opk::bgr_descriptor(frames, n, width, height, step);
    return opk_pose_submit_frames_fmt(p, &f);
}

int opk_pose_forward_frames(opk_pose* p, const uint8_t* frames, int n, int width, int height,
                            size_t step)
{
    const opk_frames f = opk::bgr_descriptor(frames, n, width, height, step);
    return opk_pose_forward_frames_fmt(p, &f);
}

}  // extern "C"

namespace {

// The pose renders on a resolved destination (BGR: the entry points below; any format:
// opk_pose_render_frames_to), inside guarded_net.

// the collected batch is the n frames about to be drawn
void check_batch(const opk::PoseHip& pose, int n)
{
    if (pose.frames() == 0) throw opk::Error(OPK_ERR_STATE, "no collected batch to render");
    if (n != pose.frames())
        throw opk::Error(OPK_ERR_STATE, "the collected batch has " +
                                            std::to_string(pose.frames()) + " frames, not " +
                                            std::to_string(n));
}

// scaleKeypoints: x and y times scaleInputToOutput, in float
void scale_keypoints(std::vector<float>& kp, double scale)
{
    const float s = (float)scale;
    if (s != 1.f)
        for (size_t i = 0; i < kp.size(); i += 3) {
            kp[i] *= s;
            kp[i + 1] *= s;
        }
}

// The keypoints of the collected batch drawn on its frames: the POSE layer and, with `part`
// ({face threshold, face alpha, hand threshold, hand alpha}; NULL: none), a layer for every
// attached extractor
void pose_render_keypoints(opk_pose* p, const opk::FrameDest& dst, const opk::FrameSource& src,
                           double scale, float threshold, float alpha, int googly_eyes,
                           int blend_original, int cast, const float* part = nullptr)
{
    const int n = src.n;
    opk::PoseHip& pose = *p->pose;
    check_batch(pose, n);
    const int parts = opk::pose_model(pose.model()).parts;
    std::vector<int> counts[3];
    std::vector<float> kp[3];
    opk_render_layer layers[3] = {};
    int nl = 0;
    for (int f = 0; f < n; ++f) {
        const int people = pose.num_people(f);
        counts[0].push_back(people);
        const auto& k = pose.keypoints(f);
        kp[0].insert(kp[0].end(), k.begin(), k.begin() + (size_t)people * parts * 3);
    }
    scale_keypoints(kp[0], scale);
    layers[nl].kind = OPK_LAYER_POSE;
    layers[nl].pose_model = pose.model();
    layers[nl].counts_host = counts[0].data();
    layers[nl].render_threshold = threshold;
    layers[nl].alpha = alpha;
    layers[nl].googly_eyes = googly_eyes;
    ++nl;
    for (int kind = 0; part && kind < 2; ++kind) {
        if (!pose.attached(kind)) continue;
        p->ctx->bind();
        const bool hand = kind == OPK_EXTRACT_HAND;
        const int hands = hand ? 2 : 1;
        std::vector<float>& v = kp[1 + kind];
        for (int f = 0; f < n; ++f) {   // a frame's left hands, then its right hands
            int first = 0, total = 0, P = 0;
            const float* all = pose.part_keypoints(kind, f, &first, &total, &P);
            const int people = pose.num_people(f);
            counts[1 + kind].push_back(hands * people);
            for (int hd = 0; hd < hands; ++hd) {
                const float* q = all + ((size_t)hd * total + first) * P * 3;
                v.insert(v.end(), q, q + (size_t)people * P * 3);
            }
        }
        scale_keypoints(v, scale);
        float* dev = static_cast<float*>(
            pose.part_render_scratch(kind, std::max<size_t>(1, v.size()) * sizeof(float)));
        if (!v.empty()) {
            OPK_HIP(hipMemcpyAsync(dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice,
                                   p->ctx->stream));
            OPK_HIP(hipStreamSynchronize(p->ctx->stream));   // `v` is pageable
        }
        layers[nl].kind = hand ? OPK_LAYER_HAND : OPK_LAYER_FACE;
        layers[nl].keypoints_dev = dev;
        layers[nl].counts_host = counts[1 + kind].data();
        layers[nl].render_threshold = part[hand ? 2 : 0];
        layers[nl].alpha = part[hand ? 3 : 1];
        ++nl;
    }
    opk::render_frames(p->ctx, dst, src, scale, layers, nl, blend_original, cast, kp[0].data(),
                       kp[0].size());
}

// one element of --part_to_show other than the keypoints (element 0: pose_render_keypoints)
void pose_render_heat(opk_pose* p, const opk::FrameDest& dst, const opk::FrameSource& src,
                      double scale, int element, float alpha_heatmap, int blend_original, int cast)
{
    const opk::PoseHip& pose = *p->pose;
    opk_render_heat heat{};
    heat.pose_model = pose.model();
    opk::render_element(pose.model(), element, &heat.kind, &heat.channel);
    check_batch(pose, src.n);
    const opk::HeatMap& lazy = pose.lazy_heat();
    // renderPose: scaleNetToOutput * scaleInputToOutput, both float; "no blending" is alpha 1,
    // so the frame is never cleared
    heat.scale_to_keep_ratio = pose.scale_net_to_output() * (float)scale;
    heat.alpha = blend_original ? alpha_heatmap : 1.f;
    opk::render_frames(p->ctx, dst, src, scale, nullptr, 0, 1, cast, nullptr, 0, &heat, &lazy);
}

void pose_render_element(opk_pose* p, const opk::FrameDest& dst, const opk::FrameSource& src,
                         double scale, int element, float threshold, float alpha_keypoint,
                         float alpha_heatmap, int googly_eyes, int blend_original, int cast)
{
    if (element == 0)
        pose_render_keypoints(p, dst, src, scale, threshold, alpha_keypoint, googly_eyes,
                              blend_original, cast);
    else
        pose_render_heat(p, dst, src, scale, element, alpha_heatmap, blend_original, cast);
}

}  // namespace

extern "C" {

int opk_pose_render_frames_fmt(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w, int out_h,
                               const opk_frames* frames, double scale, float threshold, float alpha,
                               int googly_eyes, int blend_original, int cast)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        const opk::FrameSource src = opk::frame_source(*frames);
        pose_render_keypoints(p, opk::bgr_dest(dst, dst_step, src.n, out_w, out_h), src, scale,
                              threshold, alpha, googly_eyes, blend_original, cast);
    });
}

int opk_pose_render_frames(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w, int out_h,
                           const uint8_t* frames, int n, int width, int height, size_t step,
                           double scale, float threshold, float alpha, int googly_eyes,
                           int blend_original, int cast)
{
    const opk_frames f = opk::bgr_descriptor(frames, n, width, height, step);
    return opk_pose_render_frames_fmt(p, dst, dst_step, out_w, out_h, &f, scale, threshold, alpha,
                                      googly_eyes, blend_original, cast);
}

int opk_pose_render_frames_element_fmt(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w,
                                       int out_h, const opk_frames* frames, double scale,
                                       int element, float threshold, float alpha_keypoint,
                                       float alpha_heatmap, int googly_eyes, int blend_original,
                                       int cast)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        const opk::FrameSource src = opk::frame_source(*frames);
        pose_render_element(p, opk::bgr_dest(dst, dst_step, src.n, out_w, out_h), src, scale,
                            element, threshold, alpha_keypoint, alpha_heatmap, googly_eyes,
                            blend_original, cast);
    });
}

int opk_pose_render_frames_element(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w,
                                   int out_h, const uint8_t* frames, int n, int width, int height,
                                   size_t step, double scale, int element, float threshold,
                                   float alpha_keypoint, float alpha_heatmap, int googly_eyes,
                                   int blend_original, int cast)
{
    const opk_frames f = opk::bgr_descriptor(frames, n, width, height, step);
    return opk_pose_render_frames_element_fmt(p, dst, dst_step, out_w, out_h, &f, scale, element,
                                              threshold, alpha_keypoint, alpha_heatmap, googly_eyes,
                                              blend_original, cast);
}

int opk_pose_net_input(opk_pose* p, int scale, const float** input_dev, int* net_w, int* net_h)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && input_dev, "NULL argument");
        *input_dev = p->pose->net_input(scale, net_w, net_h);
    });
}

int opk_pose_heatmaps_copy(opk_pose* p, int types, int scale_mode, float* dst_dev, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && shape, "NULL argument");
        p->pose->heatmaps_copy(types, scale_mode, dst_dev, shape);
    });
}

int opk_pose_heatmaps_copy_range(opk_pose* p, int types, int scale_mode, int frame0, int nframes,
                                 void* dst_dev, int dst_type, int shape[4])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && shape, "NULL argument");
        p->pose->heatmaps_copy_range(types, scale_mode, frame0, nframes, dst_dev, dst_type, shape);
    });
}

int opk_pose_candidates(opk_pose* p, int frame, float* candidates_host, int* counts_host)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->candidates(frame, candidates_host, counts_host);
    });
}

float opk_pose_scale_net_to_output(opk_pose* p) { return p ? p->pose->scale_net_to_output() : 0.f; }

}  // extern "C"

// ---- face / hand keypoints (op::FaceDetector, op::HandDetector, op::FaceExtractorCaffe,
//      op::HandExtractorCaffe) ----------------------------------------------------------------
struct opk_extractor {
    opk_ctx* ctx;
    std::unique_ptr<opk::KeypointExtractor> ex;
};

extern "C" {

int opk_face_detect(int pose_model, const float* keypoints, int people, int parts, float* rects)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(people == 0 || rects, "NULL rectangles");
        opk::detect_faces(pose_model, keypoints, people, parts, reinterpret_cast<opk::Rect*>(rects));
    });
}

int opk_hand_detect(int pose_model, const float* keypoints, int people, int parts, float* rects)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(people == 0 || rects, "NULL rectangles");
        opk::detect_hands(pose_model, keypoints, people, parts, reinterpret_cast<opk::Rect*>(rects));
    });
}

int opk_extractor_create(opk_ctx* ctx, opk_net* net, int kind, int net_w, int net_h,
                         opk_extractor** out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx && net && out, "NULL argument");
        // (a host-only context can create and attach one; opk_extractor_forward needs a device)
        *out = new opk_extractor{
            ctx, std::make_unique<opk::KeypointExtractor>(ctx, net->net.get(), kind, net_w, net_h)};
    });
}

int opk_extractor_destroy(opk_extractor* ex)
{
    return guarded_net([&] { delete ex; });
}

int opk_extractor_set_scales(opk_extractor* ex, int number, float range)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex, "NULL extractor");
        ex->ex->set_scales(number, range);
    });
}

int opk_extractor_set_max_batch(opk_extractor* ex, int max_batch)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex, "NULL extractor");
        ex->ex->set_max_batch(max_batch);
    });
}

int opk_extractor_parts(opk_extractor* ex) { return ex ? ex->ex->parts() : -1; }

int opk_extractor_set_heatmaps(opk_extractor* ex, int scale_mode)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex, "NULL extractor");
        ex->ex->set_heatmaps(scale_mode);
    });
}

int opk_extractor_heatmaps(opk_extractor* ex, const float** heatmaps_dev, int shape[5])
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex && heatmaps_dev && shape, "NULL argument");
        *heatmaps_dev = ex->ex->heatmaps(shape);
    });
}

int opk_extractor_forward_fmt(opk_extractor* ex, const opk_frames* frames, const float* rects,
                              const int* frame_of, int people, float* keypoints)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex && frames && (people == 0 || keypoints), "NULL argument");
        ex->ex->extract(opk::frame_source(*frames), reinterpret_cast<const opk::Rect*>(rects),
                        frame_of, people, keypoints);
    });
}

int opk_extractor_forward(opk_extractor* ex, const uint8_t* frames, int nframes, int width,
                          int height, size_t step, const float* rects, const int* frame_of,
                          int people, float* keypoints)
{
    const opk_frames f = opk::bgr_descriptor(frames, nframes, width, height, step);
    return opk_extractor_forward_fmt(ex, &f, rects, frame_of, people, keypoints);
}

int opk_extractor_crop_count(opk_extractor* ex) { return ex ? ex->ex->crops() : -1; }

int opk_extractor_crop(opk_extractor* ex, int i, double* matrix, const float** input_dev)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ex, "NULL extractor");
        OPK_CHECK_ARG(i >= 0 && i < ex->ex->crops(), "crop index out of range");
        const auto* k = ex->ex.get();
        if (matrix) std::memcpy(matrix, k->crop_matrix(i), 6 * sizeof(double));
        if (input_dev) {
            // crops are laid out [crops][3][net_h][net_w]
            // (NULL after a pipeline-stage run: only one net batch's crops are ever staged)
            const float* in = k->crop_inputs();
            *input_dev = in ? in + (size_t)i * 3 * k->net_w() * k->net_h() : nullptr;
        }
    });
}

// ---- face / hand stages of the pose pipeline ---------------------------------------------------
int opk_pose_attach_extractor(opk_pose* p, opk_extractor* ex)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && ex, "NULL argument");
        p->pose->attach_extractor(ex->ex.get());
    });
}

int opk_pose_detach_extractor(opk_pose* p, int kind)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->detach_extractor(kind);
    });
}

int opk_pose_part_rectangles(opk_pose* p, int kind, int frame, float* rects_host)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        const opk::Rect* r = p->pose->part_rectangles(kind, frame);
        const size_t count = (size_t)p->pose->num_people(frame) * (kind == OPK_EXTRACT_HAND ? 2 : 1);
        OPK_CHECK_ARG(count == 0 || rects_host, "NULL rectangles");
        if (count) std::memcpy(rects_host, r, count * sizeof(opk::Rect));
    });
}

int opk_pose_part_keypoints(opk_pose* p, int kind, int frame, float* keypoints_host, int max_people)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        int first = 0, total = 0, parts = 0;
        const float* kp = p->pose->part_keypoints(kind, frame, &first, &total, &parts);
        const int people = std::min(max_people, p->pose->num_people(frame));
        if (people <= 0) return;
        OPK_CHECK_ARG(keypoints_host, "NULL keypoints");
        const size_t person = (size_t)parts * 3;
        for (int hd = 0; hd < (kind == OPK_EXTRACT_HAND ? 2 : 1); ++hd)
            std::memcpy(keypoints_host + (size_t)hd * people * person,
                        kp + ((size_t)hd * total + first) * person, people * person * sizeof(float));
    });
}

int opk_pose_read_part_times(opk_pose* p, int kind, int* batches, int* crops, double* host_ms,
                             double* wait_ms)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->read_part_times(kind, batches, crops, host_ms, wait_ms);
    });
}

int opk_pose_render_frames_parts_fmt(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w,
                                     int out_h, const opk_frames* frames, double scale,
                                     float threshold, float alpha, int googly_eyes,
                                     int blend_original, int cast, float face_threshold,
                                     float face_alpha, float hand_threshold, float hand_alpha)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        const opk::FrameSource src = opk::frame_source(*frames);
        const float part[4] = {face_threshold, face_alpha, hand_threshold, hand_alpha};
        pose_render_keypoints(p, opk::bgr_dest(dst, dst_step, src.n, out_w, out_h), src, scale,
                              threshold, alpha, googly_eyes, blend_original, cast, part);
    });
}

int opk_pose_render_frames_to(opk_pose* p, const opk_frames_out* dst, const opk_frames* frames,
                              double scale, int element, float threshold, float alpha_keypoint,
                              float alpha_heatmap, int googly_eyes, int blend_original, int cast,
                              const float* part_params)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        OPK_CHECK_ARG(frames, "NULL frames");
        OPK_CHECK_ARG(dst, "NULL destination");
        const opk::FrameSource src = opk::frame_source(*frames);
        const opk::FrameDest d = opk::frame_dest_for(*dst, src);
        if (!part_params) {
            pose_render_element(p, d, src, scale, element, threshold, alpha_keypoint, alpha_heatmap,
                                googly_eyes, blend_original, cast);
            return;
        }
        OPK_CHECK_ARG(element == 0, "face / hand layers are drawn with the keypoints (element 0)");
        pose_render_keypoints(p, d, src, scale, threshold, alpha_keypoint, googly_eyes,
                              blend_original, cast, part_params);
    });
}

int opk_pose_render_frames_parts(opk_pose* p, uint8_t* dst, size_t dst_step, int out_w, int out_h,
                                 const uint8_t* frames, int n, int width, int height, size_t step,
                                 double scale, float threshold, float alpha, int googly_eyes,
                                 int blend_original, int cast, float face_threshold,
                                 float face_alpha, float hand_threshold, float hand_alpha)
{
    const opk_frames f = opk::bgr_descriptor(frames, n, width, height, step);
    return opk_pose_render_frames_parts_fmt(p, dst, dst_step, out_w, out_h, &f, scale, threshold,
                                            alpha, googly_eyes, blend_original, cast,
                                            face_threshold, face_alpha, hand_threshold, hand_alpha);
}

}  // extern "C"

// ---- person ids across frames (host/track.h, kernels/track.hip) ---------------------------------
struct opk_tracker {
    opk_ctx* ctx;
    std::unique_ptr<opk::Tracker> t;
};

extern "C" {

int opk_pyramid_layout(int width, int height, int levels, int* level_w, int* level_h,
                       size_t* level_offset, size_t* frame_bytes)
{
    return guarded_net([&] {
        const opk::PyramidLayout L = opk::pyramid_layout(width, height, levels);
        for (int l = 0; l < levels; ++l) {
            if (level_w) level_w[l] = L.w[l];
            if (level_h) level_h[l] = L.h[l];
            if (level_offset) level_offset[l] = L.at[l];
        }
        if (frame_bytes) *frame_bytes = L.frame;
    });
}

int opk_pyramid_build(opk_ctx* ctx, void* pyramid_dev, const opk_frames* frames, int levels)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx, "NULL ctx");
        OPK_CHECK_ARG(frames, "NULL frames");
        const opk::FrameSource src = opk::frame_source(*frames);
        OPK_CHECK_ARG(src.w > 0 && src.h > 0, "empty frame");
        const opk::PyramidLayout L = opk::pyramid_layout(src.w, src.h, levels);
        if (src.n == 0) return;
        ctx->bind();
        opk::launch_pyramid(static_cast<uint8_t*>(pyramid_dev), L, src, ctx->stream);
    });
}

int opk_pyramid_level(opk_ctx* ctx, float* dst_dev, const void* pyramid_dev, int n, int width,
                      int height, int levels, int level)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx, "NULL ctx");
        const opk::PyramidLayout L = opk::pyramid_layout(width, height, levels);
        OPK_CHECK_ARG(n >= 0, "negative frame count");
        OPK_CHECK_ARG(level >= 0 && level < levels, "no such pyramid level");
        if (n == 0) return;
        ctx->bind();
        opk::launch_pyramid_level(dst_dev, static_cast<const uint8_t*>(pyramid_dev), L, n, level,
                                  ctx->stream);
    });
}

int opk_lk_points(opk_ctx* ctx, const void* pyramid_dev, int n_frames, const void* carry_dev,
                  int width, int height, opk_lk_point* points_dev, int npoints)
{
    static_assert(sizeof(opk_lk_point) == sizeof(opk::LkPoint), "opk_lk_point is kernels.h's LkPoint");
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx, "NULL ctx");
        const opk::PyramidLayout L = opk::pyramid_layout(width, height, opk::kPyramidLevels);
        OPK_CHECK_ARG(npoints >= 0 && n_frames >= 0, "negative count");
        if (npoints == 0) return;
        ctx->bind();
        opk::launch_lk_points(reinterpret_cast<opk::LkPoint*>(points_dev), npoints,
                              static_cast<const uint8_t*>(pyramid_dev), n_frames,
                              static_cast<const uint8_t*>(carry_dev), L, ctx->stream);
    });
}

int opk_tracker_create(opk_ctx* ctx, float confidence, float inlier_ratio, float distance,
                       int frames_to_delete, opk_tracker** out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(ctx && out, "NULL argument");
        *out = new opk_tracker{ctx, std::make_unique<opk::Tracker>(ctx, confidence, inlier_ratio,
                                                                   distance, frames_to_delete)};
    });
}

int opk_tracker_destroy(opk_tracker* t)
{
    return guarded_net([&] {
        if (!t) return;
        if (t->ctx->device >= 0) t->ctx->bind();
        delete t;
    });
}

int opk_tracker_reset(opk_tracker* t)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(t, "NULL tracker");
        t->t->reset();
    });
}

int opk_tracker_update(opk_tracker* t, const opk_frames* frames, const float* keypoints_host,
                       const int* people_per_frame, int parts, long long* ids_host)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "ids are 64-bit");
    return guarded_net([&] {
        OPK_CHECK_ARG(t, "NULL tracker");
        OPK_CHECK_ARG(frames, "NULL frames");
        const opk::FrameSource src = opk::frame_source(*frames);
        OPK_CHECK_ARG(parts > 0, "no parts");
        if (src.n == 0) return;
        t->t->build(0, src, t->ctx->stream);
        t->t->update(0, keypoints_host, people_per_frame, src.n, parts,
                     reinterpret_cast<int64_t*>(ids_host));
    });
}

int opk_tracker_set_timing(opk_tracker* t, int enable)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(t, "NULL tracker");
        t->t->set_timing(enable != 0);
    });
}

int opk_tracker_read_times(opk_tracker* t, int* batches, double* pyramid_ms, double* lk_ms,
                           double* host_ms, size_t* device_bytes)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(t, "NULL tracker");
        t->t->read_times(batches, pyramid_ms, lk_ms, host_ms);
        if (device_bytes) *device_bytes = t->t->device_bytes();
    });
}

int opk_pose_attach_tracker(opk_pose* p, opk_tracker* t)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && t, "NULL argument");
        p->pose->attach_tracker(t->t.get());
    });
}

int opk_pose_detach_tracker(opk_pose* p)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->detach_tracker();
    });
}

int opk_pose_person_ids(opk_pose* p, int frame, long long* ids_host)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        const std::vector<int64_t>& ids = p->pose->person_ids(frame);
        OPK_CHECK_ARG(ids.empty() || ids_host, "NULL ids");
        if (!ids.empty()) std::memcpy(ids_host, ids.data(), ids.size() * sizeof(int64_t));
    });
}

int opk_pose_set_views(opk_pose* p, const opk_rig* rig)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        if (!rig) {
            p->pose->set_views(nullptr);
            return;
        }
        const opk::TriRig r = opk::make_rig(rig);
        p->pose->set_views(&r);
    });
}

int opk_pose_keypoints_3d(opk_pose* p, int step, int kind, float* xyz_host, int* status)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && xyz_host && status, "NULL argument");
        int parts = 0;
        const float* xyz = p->pose->keypoints_3d(step, kind, &parts, status);
        std::memcpy(xyz_host, xyz, (size_t)parts * 4 * sizeof(float));
    });
}

int opk_pose_set_undistort(opk_pose* p, const opk_cameras* cams)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        if (!cams) {
            p->pose->set_undistort(nullptr);
            return;
        }
        const opk::UndistortCameras c = opk::make_cameras(cams);
        p->pose->set_undistort(&c);
    });
}

int opk_pose_undistorted_frames(opk_pose* p, opk_frames* out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && out, "NULL argument");
        const opk::FrameSource& f = p->pose->undistorted_frames();
        *out = opk_frames{};
        out->format = OPK_FRAMES_BGR;
        out->n = f.n;
        out->width = f.w;
        out->height = f.h;
        out->plane[0] = f.plane[0];
        out->step[0] = f.step;
        out->frame_bytes[0] = f.frame[0];
    });
}

int opk_pose_set_orientation(opk_pose* p, int rotate, int flip)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->set_orientation(opk::make_orientation(rotate, flip));
    });
}

int opk_pose_oriented_frames(opk_pose* p, opk_frames* out)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p && out, "NULL argument");
        const opk::FrameSource& f = p->pose->oriented_frames();
        *out = opk_frames{};
        out->format = f.format;
        out->n = f.n;
        out->width = f.w;
        out->height = f.h;
        const int planes = f.format == OPK_FRAMES_BGR ? 1 : f.format == OPK_FRAMES_NV12 ? 2 : 3;
        for (int i = 0; i < planes; ++i) {
            out->plane[i] = f.plane[i];
            out->step[i] = i == 0 ? f.step : f.cstep;
            out->frame_bytes[i] = f.frame[i];
        }
    });
}

int opk_pose_read_track_times(opk_pose* p, int* batches, double* pyramid_ms, double* lk_ms,
                              double* host_ms)
{
    return guarded_net([&] {
        OPK_CHECK_ARG(p, "NULL pose");
        p->pose->read_track_times(batches, pyramid_ms, lk_ms, host_ms);
    });
}

}  // extern "C"
