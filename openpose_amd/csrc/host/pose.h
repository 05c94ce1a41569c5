// pose.h -- PoseHip: the op::PoseExtractorCaffe::forwardPass replacement for a batch of frames.
#pragma once
#include <memory>
#include <vector>

#include "connector.h"
#include "context.h"
#include "extract.h"
#include "net.h"
#include "pool.h"
#include "track.h"
#include "triangulate.h"
#include "orient.h"
#include "undistort.h"

namespace opk {

// Two-stage pipeline, the single-GPU equivalent of the reference's worker threads
// (WPoseExtractor feeding the CPU-side consumers through WQueue, wrapper/wrapperAuxiliary.hpp):
//   submit  -- enqueue the device work of a batch (net, NMS, PAF scores, D2H of the results) on
//              the context stream and return;
//   collect -- wait for the oldest submitted batch and assemble its people on the host.
// With one batch in flight, the host assembly of batch i overlaps the device work of batch i+1.
// Stream contract: every input (frames, net inputs, an injected net output, the overlay) is read
// in order after the work the caller queued on the context stream before the submit call.
// forward() = submit + collect.
class PoseHip {
public:
    // pose_model: PoseModel id (pose_model.h); semantics: kConnectCpu / kConnectGpu (connector.h)
    PoseHip(Context* ctx, NetHip* net, bool maximize_positives, int pose_model = 0,
            int semantics = kConnectCpu);
    ~PoseHip();

    void set_property(int prop, double v);
    // heat-map semantics of resize + NMS (maps.h: kMapsCpu, kMapsCuda)
    void set_map_semantics(int maps);
    int map_semantics() const { return maps_; }
    double property(int prop) const { return props_[prop]; }
    void set_overlay(const float* overlay) { overlay_ = overlay; }
    // --upsampling_ratio (flags.hpp:136): heat maps at round(ratio x net output) instead of the net
    // input size; <= 0 is the default (the net's decrease factor, poseExtractorCaffe.cpp:47-54)
    void set_upsampling_ratio(float ratio);
    float upsampling_ratio() const { return upsampling_; }

    void forward(const float* frames, int n, int net_h, int net_w, int prod_w, int prod_h);
    void forward_net_output(const float* net_out, int n, int out_h, int out_w, int net_h,
                            int net_w, int prod_w, int prod_h);
    void submit(const float* frames, int n, int net_h, int net_w, int prod_w, int prod_h);
    void submit_net_output(const float* net_out, int n, int out_h, int out_w, int net_h,
                           int net_w, int prod_w, int prod_h);
    // multi-scale (poseExtractorCaffe.cpp:240-245, resizeAndMergeBase.cpp:55-106): frames[i] is
    // the [n][3][net_hw[2i]][net_hw[2i+1]] net input of scale i; scale 0 sets the heat-map size
    void submit_multi(const float* const* frames, const int* net_hw, int nscales, int n,
                      int prod_w, int prod_h);
    // raw frames (the reference's full per-frame path: ScaleAndSizeExtractor -> CvMatToOpInput ->
    // PoseExtractorCaffe): n BGR uint8 frames [h][step bytes] on device, prepared on the GPU for
    // every scale of set_input(), then the net per scale and the merged post-processing
    void set_input(int net_w, int net_h, float dyn, int scale_number, double scale_gap);
    // (frames: BGR, or NV12 / I420 converted inside the warps)
    void submit_frames(const FrameSource& frames);
    void forward_frames(const FrameSource& frames);
    // net input of scale i of the last submit_frames ([n][3][h][w] fp32 device; w/h may be NULL)
    const float* net_input(int i, int* w, int* h) const;
    int collect();                       // frames of the collected batch
    int pending() const { return count_; }

    // results of the last collected batch
    int frames() const { return (int)people_.size(); }
    int num_people(int f) const { return people_.at(f); }
    const std::vector<float>& keypoints(int f) const { return kp_.at(f); }
    const std::vector<float>& scores(int f) const { return ks_.at(f); }
    // full-resolution heat maps of the last collected batch, materialised on first request (the
    // pipeline evaluates them lazily from the net output: HeatMap in kernels.h); only while no
    // later batch is in flight (its net forward overwrites the net output)
    float* heatmaps(int shape[4]);
    void heatmap_size(int shape[4]) const;   // the last collected batch's, nothing materialised
    // the last collected batch's lazy map itself (the batch render's heat layer reads it); an
    // OPK_ERR_STATE error under heatmaps()' conditions; nothing is materialised
    const HeatMap& lazy_heat() const;
    float* peaks(int shape[4]) const;
    // PoseExtractorNet::getHeatMapsCopy (poseExtractorNet.cpp:106-244) for every frame of the last
    // collected batch: types bit 0 parts, bit 1 background, bit 2 PAFs (in that order), scale_mode
    // an op::ScaleMode value; dst [n][channels of the types][H][W] device (NULL: shape only)
    void heatmaps_copy(int types, int scale_mode, float* dst, int shape[4]);
    // the same values of frames frame0 .. frame0 + nframes - 1 (nframes -1: to the batch's end)
    // straight from the lazy map (heat_out.hip): heat_ is neither allocated nor read.  dst_type
    // OPK_F32, or OPK_U8 (scale_mode UnsignedChar only): min(value, 255)
    void heatmaps_copy_range(int types, int scale_mode, int frame0, int nframes, void* dst,
                             int dst_type, int shape[4]);
    // PoseExtractorNet::getCandidatesCopy (:246-282): peaks of one frame, x/y * scaleNetToOutput;
    // out [parts][kMaxPeaks][3], counts [parts]
    void candidates(int frame, float* out, int* counts) const;
    float scale_net_to_output() const { return scale_net_to_output_; }
    // device time of the post-processing of every submitted batch (overlay add, NMS, PAF
    // integrals: the work after the net forward), HIP events on the context stream
    void set_timing(bool on) { timer_.on = on; }
    void read_timing(int* count, double* total_ms) { timer_.read(count, total_ms); }
    // host time of the collects since the last read: waiting for the batch's device results
    // (D2H copies behind its post-processing) and assembling its people on the pool's threads
    void read_collect_times(int* count, double* wait_ms, double* assembly_ms);
    int assembly_workers() const { return pool_ ? pool_->workers() : assembly_threads(); }
    int model() const { return model_; }

    // Face / hand stages (the reference's WFaceDetector + WFaceExtractorNet, WHandDetector +
    // WHandExtractorNet workers behind WPoseExtractor): at most one extractor per kind
    // (KeypointExtractor::kFace / kHand), of this context, over a net that is not the pose net.
    // While one is attached only submit_frames / forward_frames are accepted, and collect() runs,
    // after the people assembly of batch i: rectangles per frame from the batch's keypoints
    // (detect_faces / detect_hands), concatenated in frame order, then extract(..., chunked) on
    // batch i's frames -- queued on the context stream behind the nets of batch i + 1, which the
    // earlier submit enqueued.  The frame buffer of a submitted batch must therefore stay
    // unchanged until that batch is collected.
    void attach_extractor(KeypointExtractor* ex);
    void detach_extractor(int kind);
    // (an extractor destroyed while attached counts as detached from then on)
    bool attached(int kind) const
    {
        return kind >= 0 && kind < 2 && part_[kind].ex != nullptr && !part_[kind].alive.expired();
    }
    // results of the last collected batch (an OPK_ERR_STATE error without extractor or batch):
    // rects [people] (face) or [people][2] (hand) of frame f
    const Rect* part_rectangles(int kind, int f) const;
    // keypoints of frame f: the whole batch's array as extract() fills it (face [total][P][3],
    // hand [2][total][P][3]), the frame's first person in it and the batch's people
    const float* part_keypoints(int kind, int f, int* first, int* total, int* parts) const;
    // since the last read: batches and crops run, host ms for rectangles, crop validity and
    // tables, ms waiting for the device
    void read_part_times(int kind, int* batches, int* crops, double* host_ms, double* wait_ms);
    // Person ids (the reference's --identification: PoseExtractor::extractIds behind the pose
    // worker): one Tracker of this context, under the rules of the face / hand stages -- raw-frame
    // path only, no attach / detach with batches in flight, the submitted frames stay unchanged
    // until collected.  submit_frames queues the batch's pyramid on the context stream; collect()
    // runs Tracker::update on the batch's keypoints after run_parts, on the context stream.
    void attach_tracker(Tracker* t);
    void detach_tracker();
    bool tracker_attached() const { return tracker_ != nullptr && !tracker_alive_.expired(); }
    // ids of frame f of the last collected batch (an OPK_ERR_STATE error without tracker or batch)
    const std::vector<int64_t>& person_ids(int f) const;
    void read_track_times(int* batches, double* pyramid_ms, double* lk_ms, double* host_ms);
    // 3-D keypoints (the reference's --3d: WPoseTriangulation behind the pose, face and hand
    // workers): while a rig is set a batch of n frames is n / V time steps, frame t*V + v the view
    // v of step t (submit checks n and the frame size against the rig); collect(), after
    // run_parts, uploads person 0 of every frame, runs triangulate() once per array kind (body,
    // and face / left hand / right hand where attached) on the context stream and downloads the
    // results.  Set / clear (nullptr) only with no batch in flight.
    void set_views(const TriRig* rig);
    bool views_set() const { return views_.views > 0; }
    // [parts][4] and the status of one step of the last collected batch; kind 0 body, 1 face,
    // 2 left hand, 3 right hand (an OPK_ERR_STATE error without views, batch or that extractor)
    const float* keypoints_3d(int step, int kind, int* parts, int* status) const;
    // Undistortion (the reference's --frame_undistort, which its producer runs on every frame
    // before any worker sees it): while cameras are set, submit_frames first remaps the batch,
    // frame f through the maps of view f % V, into the BGR buffer of the batch's slot; the warp,
    // the tracker's pyramid, the face / hand crops and the rig's size check read that buffer
    // (Slot::raw describes it).  n not a multiple of V or another frame size is OPK_ERR_ARG at
    // submit.  130 frames of 1280x720 are 360 MB per slot; clearing frees both slots' buffers.
    // Set / clear (nullptr) only with no batch in flight.
    void set_undistort(const UndistortCameras* cams);
    bool undistort_set() const { return undist_.views() > 0; }
    // the collected batch's buffer, valid until the second submit after that batch's (an
    // OPK_ERR_STATE error without cameras or without a batch collected with them)
    const FrameSource& undistorted_frames() const;
    // Orientation (the reference's --frame_rotate / --frame_flip, which its producer applies right
    // after the undistortion): while one is set, submit_frames permutes the batch -- the
    // undistorted buffer when cameras are set too -- into a buffer of the batch's slot, in the
    // source's format with tight rows; scale_and_size, the warp, the tracker's pyramid, the face /
    // hand crops and the rig's size check take the oriented description and size, the cameras'
    // check the source size.  (0, false) clears the stage and frees both slots' buffers.  Set /
    // clear only with no batch in flight.
    void set_orientation(const Orientation& o);
    bool orientation_set() const { return orient_.set(); }
    // the collected batch's oriented buffer, under undistorted_frames()' lifetime rule (an
    // OPK_ERR_STATE error without the stage or without a batch collected with it)
    const FrameSource& oriented_frames() const;
    // device scratch of the face / hand layers of a batch render (grows, never shrinks)
    void* part_render_scratch(int kind, size_t bytes) { return part_dev_[kind & 1].get(bytes); }

    static constexpr int kMaxPeaks = kPoseMaxPeople;   // peaks blob [parts][128][3]
    static constexpr int kRecordHead = 16384;          // record floats copied eagerly per frame
    // host threads assembling a batch's people: at most this many, and at most the CPUs of the
    // process's affinity mask (assembly_threads)
    static constexpr int kAssemblyThreads = 16;
    static int assembly_threads();

private:
    struct Slot {
        DevBuf peaks, records;
        HostBuf hpeaks, hrecords;
        hipEvent_t done = nullptr;
        int n = 0, H = 0, W = 0;
        float scale = 1.f;
        HeatMap heat{};
        FrameSource raw{};   // a copy of the batch's frame description (submit_frames), for the
                             // face / hand stages; plane[0] NULL: none
        DevBuf undist;       // the batch's undistorted frames, tight BGR (set_undistort): what raw
                             // describes then
        DevBuf orient;       // the batch's oriented frames (set_orientation): what raw describes then
        FrameSource und{}, ori{};   // what undist / orient hold of this batch; plane[0] NULL: nothing
    };
    struct Part {
        KeypointExtractor* ex = nullptr;
        std::weak_ptr<void> alive;    // KeypointExtractor::liveness
        int parts = 0;
        std::vector<Rect> rects;      // the collected batch's, frame after frame
        std::vector<float> kp;        // as extract() fills it
        int batches = 0, crops = 0;
        double host_ms = 0., wait_ms = 0.;
    };
    Part part_[2];
    DevBuf part_dev_[2];
    std::vector<int> part_first_;     // [n + 1]: first person of each frame in the batch's arrays
    bool parts_valid_ = false;
    FrameSource cur_raw_{};           // set by submit_frames for the submit it makes
    FrameSource cur_und_{}, cur_ori_{};   // likewise: the stages' buffers of that batch
    bool any_attached() const { return attached(0) || attached(1); }
    void need_frames() const;         // the OPK_ERR_STATE of a submit without frames
    void run_parts(const Slot& sl);
    Tracker* tracker_ = nullptr;
    std::weak_ptr<void> tracker_alive_;   // Tracker::liveness
    std::vector<std::vector<int64_t>> ids_;   // the collected batch's, per frame
    bool ids_valid_ = false;
    void run_tracker(const Slot& sl, int slot);
    TriRig views_{};                  // views == 0: none
    struct Array3d {
        int parts = 0;                // 0: the kind was not run
        std::vector<float> xyz;       // [steps][parts][4]
        std::vector<int> status;      // [steps]
    };
    Array3d v3d_[4];
    int v3d_steps_ = 0;
    bool v3d_valid_ = false;
    DevBuf v3d_dev_;
    HostBuf v3d_host_;
    void check_views(int n, int w, int h) const;   // the OPK_ERR_ARG of a submit against the rig
    UndistortCameras undist_;         // no views: none
    FrameSource undist_out_{};        // the collected batch's undistorted frames
    bool undist_valid_ = false;
    Orientation orient_{};            // not set(): none
    FrameSource orient_out_{};        // the collected batch's oriented frames
    bool orient_valid_ = false;
    void run_views(const Slot& sl);
    struct NetOutput {
        const float* ptr;
        int h, w;
    };
    void submit_outputs(const NetOutput* outs, int nscales, int n, int net_h, int net_w,
                        int prod_w, int prod_h, bool own_net);
    size_t record_floats() const;        // per frame: 1 + every candidate pair of the model

    Context* ctx_;
    NetHip* net_;
    std::weak_ptr<void> net_alive_;   // NetHip::liveness (the net may be destroyed first)
    NetHip* live_net() const;         // net_, or an error if it was destroyed
    // set_input(): --net_resolution, --net_resolution_dynamic, --scale_number, --scale_gap
    int in_net_w_ = -1, in_net_h_ = 368, scale_number_ = 1;
    float dyn_ = 1.f;
    double scale_gap_ = 0.25;
    DevBuf inputs_[kMaxResizeSources];
    int input_hw_[2 * kMaxResizeSources] = {};
    int inputs_n_ = 0;
    bool maximize_positives_;
    int model_, semantics_;
    int maps_ = 0;                              // kMapsCpu
    float map_ratios_[kMaxResizeSources] = {};  // scaleInputToNetInputs of the raw-frame path
    bool have_ratios_ = false;
    double props_[5];
    const float* overlay_ = nullptr;
    float upsampling_ = 0.f;
    hipStream_t copy_ = nullptr;         // D2H of collected batches (overlaps the next batch)
    // When this PoseHip runs the net itself (submit, submit_multi, submit_frames), the
    // post-processing of a batch (overlay, NMS, PAF integrals) runs on post_, ordered after the
    // batch's nets on the context stream.  Everything the caller enqueues on the context stream
    // -- frame uploads included -- stays ordered before the next batch's warp and nets, and the
    // next batch's warp overlaps this batch's post-processing.  The nets alternate between two
    // output buffers per input shape (NetHip::select_output; NET_OUT_ALT=0: one), and before a
    // forward the context stream waits for those of the last two recorded post-processings that
    // read the buffer it is about to write (NetHip::note_reader, which also orders a direct
    // opk_net_forward of the same net after them) -- so batch i+1's nets start while batch i's
    // post-processing still runs.  post_ is a side stream of the context (opk_sync waits for it).
    // POST_STREAM=0: all on the context stream.
    // The injection path (submit_net_output: a caller-owned net output) stays on the context
    // stream, so a caller may rewrite that buffer on its stream after submit.
    hipStream_t post_ = nullptr;
    hipEvent_t nets_done_ = nullptr, post_done_[2] = {};
    int post_count_ = 0;                     // post-processings recorded on post_
    hipStream_t post_stream(bool own_net);   // the stream a batch's post-processing runs on
    void wait_post(hipStream_t s);           // s after the last recorded post-processing
    // switch the shape's output buffer for its next forward (alternate) and plan the shape
    void next_output(int n, int h, int w, bool alternate);
    DevBuf cand_;                            // NMS candidate counters (zeroed once, self-resetting)
    // multi-scale: the nets of scales 1.. run on their own streams beside scale 0's
    hipStream_t scale_streams_[kMaxResizeSources - 1] = {};
    hipEvent_t fork_ = nullptr, join_[kMaxResizeSources - 1] = {};
    EventTimer timer_;

    Slot slots_[2];
    int head_ = 0, count_ = 0, last_ = -1;
    HostBuf overflow_;                   // records longer than the copied head (pinned)
    size_t record_head_ = kRecordHead;   // record floats per frame copied eagerly (adaptive)
    int peak_rows_ = kMaxPeaks + 1;      // peak rows per part copied eagerly (adaptive)
    // people assembly: worker threads (started by the first multi-frame collect) and one
    // scratch per worker
    std::unique_ptr<WorkerPool> pool_;
    int collect_count_ = 0;
    double collect_wait_ms_ = 0., collect_assembly_ms_ = 0.;
    std::vector<AssemblyScratch> scratch_;

    float scale_net_to_output_ = 1.f;
    int n_ = 0, hh_ = 0, hw_ = 0;
    bool heat_valid_ = false;
    DevBuf heat_, heat_sel_;
    std::vector<int> people_;
    std::vector<std::vector<float>> kp_, ks_;
};

// resizeGetScaleFactor (src/openpose/utilities/openCv.cpp:182-195)
double resize_scale_factor(int iw, int ih, int tw, int th);

}  // namespace opk
