// track.h -- person ids across frames: op::PersonIdExtractor (--identification) for batches
// (src/openpose/tracking/personIdExtractor.cpp:83-290, 429-476); the definition: include/opk.h.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <vector>

#include "context.h"

namespace opk {

// matchLKAndOPGreedy (personIdExtractor.cpp:168-290) up to the id assignment: entries
// [n_entries][parts][3] and people [n_people][parts][3] hold (x, y, status); entry_ids strictly
// ascending.  ids_out [n_people]; *next_id is advanced by the people no entry matched.  Pure host.
void match_people(const float* entries, const int64_t* entry_ids, int n_entries, const float* people,
                  int n_people, int parts, float inlier_ratio, float distance, int width, int height,
                  int64_t* next_id, int64_t* ids_out);

// The tracker's bookkeeping.  A batch goes through in two steps so that the pose pipeline can put
// them at submit and at collect: build() queues the batch's pyramid into one of two slots (two
// batches may be in flight), update() runs Lucas-Kanade and the matching of the frames in order.
// Fresh points -- frame f - 1's detections into frame f, and the carried-in frame's into frame 0 --
// are all known when update() starts and go in one launch; entries nobody re-detected are
// propagated while walking the frames, in one small launch per frame that has any.
class Tracker {
public:
    Tracker(Context* ctx, float confidence, float inlier_ratio, float distance, int frames_to_delete);
    ~Tracker();
    Context* context() const { return ctx_; }
    std::shared_ptr<void> liveness() const { return alive_; }

    void reset();   // forget ids, entries and the previous frame
    void build(int slot, const FrameSource& frames, hipStream_t stream);
    // keypoints: the people of every frame one after the other [sum(people)][parts][3] (x, y,
    // score); ids_out [sum(people)].  The frames are those of the slot's last build().
    void update(int slot, const float* keypoints, const int* people, int nframes, int parts,
                int64_t* ids_out);

    void set_timing(bool on) { pyr_timer_.on = lk_timer_.on = on; }
    // since the last read: update() calls, device ms of their pyramids and LK launches, host ms
    // of the walk (capture, bookkeeping, matching; without the waits for the device)
    void read_times(int* batches, double* pyramid_ms, double* lk_ms, double* host_ms);
    size_t device_bytes() const;   // pyramids, carried frame and point records held

private:
    struct Entry {
        std::vector<float> pts;   // [parts][3] (x, y, status)
        int counter = 0;
        int src = -1;             // counter 0: the person of the frame before that it was taken from
    };
    // points of `count` people [parts][3] from frame fi to fj of the slot: LK in place
    void propagate(int slot, float* pts, size_t npoints, const int* frame_i, const int* frame_j);

    Context* ctx_;
    std::shared_ptr<void> alive_;
    float confidence_, inlier_ratio_, distance_;
    int frames_to_delete_;

    int64_t next_id_ = 0;
    std::map<int64_t, Entry> entries_;   // ascending ids: the order ties are resolved in
    std::vector<float> last_capture_;    // the last frame's people (x, y, status)
    bool has_prev_ = false;
    int parts_ = 0;

    PyramidLayout layout_{};
    DevBuf pyr_[2], carry_, points_;
    int slot_n_[2] = {0, 0};
    HostBuf hpoints_;
    EventTimer pyr_timer_, lk_timer_;
    int batches_ = 0;
    double host_ms_ = 0.;
};

}  // namespace opk
