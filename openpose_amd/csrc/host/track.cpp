// track.cpp -- Tracker: op::PersonIdExtractor::extractIds (personIdExtractor.cpp:429-476) with
// updateLK / initializeLK (:83-161) for batches of frames; the definition: include/opk.h.
#include "track.h"

#include <chrono>
#include <cstring>

namespace opk {

namespace {
double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

Tracker::Tracker(Context* ctx, float confidence, float inlier_ratio, float distance,
                 int frames_to_delete)
    : ctx_(ctx), alive_(std::make_shared<int>(0)), confidence_(confidence),
      inlier_ratio_(inlier_ratio), distance_(distance), frames_to_delete_(frames_to_delete)
{
    OPK_CHECK_ARG(ctx != nullptr, "NULL context");
}

Tracker::~Tracker() = default;

void Tracker::reset()
{
    next_id_ = 0;
    entries_.clear();
    last_capture_.clear();
    has_prev_ = false;
    parts_ = 0;
}

size_t Tracker::device_bytes() const
{
    return pyr_[0].bytes + pyr_[1].bytes + carry_.bytes + points_.bytes;
}

void Tracker::read_times(int* batches, double* pyramid_ms, double* lk_ms, double* host_ms)
{
    double p = 0., l = 0.;
    if (ctx_->device >= 0) {
        ctx_->bind();
        pyr_timer_.read(nullptr, &p);
        lk_timer_.read(nullptr, &l);
    }
    if (batches) *batches = batches_;
    if (pyramid_ms) *pyramid_ms = p;
    if (lk_ms) *lk_ms = l;
    if (host_ms) *host_ms = host_ms_;
    batches_ = 0;
    host_ms_ = 0.;
}

void Tracker::build(int slot, const FrameSource& frames, hipStream_t stream)
{
    OPK_CHECK_ARG(slot == 0 || slot == 1, "slot 0 or 1");
    OPK_CHECK_ARG(frames.n > 0 && frames.w > 0 && frames.h > 0 && frames.plane[0], "empty frames");
    ctx_->bind();
    const PyramidLayout L = pyramid_layout(frames.w, frames.h, kPyramidLevels);
    if (has_prev_ && (L.w[0] != layout_.w[0] || L.h[0] != layout_.h[0]))
        throw Error(3, "the tracker holds a frame of another size: reset it first");
    if (slot_n_[slot ^ 1] > 0 && (L.w[0] != layout_.w[0] || L.h[0] != layout_.h[0]))
        throw Error(3, "a batch of another frame size is in flight");
    layout_ = L;
    uint8_t* pyr = static_cast<uint8_t*>(pyr_[slot].get((size_t)frames.n * L.frame));
    pyr_timer_.begin(stream);
    launch_pyramid(pyr, L, frames, stream);
    pyr_timer_.end(stream);
    slot_n_[slot] = frames.n;
}

void Tracker::propagate(int slot, float* pts, size_t npoints, const int* frame_i, const int* frame_j)
{
    if (npoints == 0) return;
    OPK_CHECK_ARG(npoints <= (size_t)1 << 30, "too many points");
    const hipStream_t s = ctx_->stream;
    const size_t bytes = npoints * sizeof(LkPoint);
    LkPoint* h = static_cast<LkPoint*>(hpoints_.get(bytes));
    for (size_t i = 0; i < npoints; ++i)
        h[i] = LkPoint{frame_i[i], frame_j[i], pts[3 * i], pts[3 * i + 1], (int)pts[3 * i + 2]};
    LkPoint* d = static_cast<LkPoint*>(points_.get(bytes));
    OPK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    lk_timer_.begin(s);
    launch_lk_points(d, (int)npoints, static_cast<const uint8_t*>(pyr_[slot].ptr), slot_n_[slot],
                     has_prev_ ? static_cast<const uint8_t*>(carry_.ptr) : nullptr, layout_, s);
    lk_timer_.end(s);
    OPK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
    OPK_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < npoints; ++i) {
        pts[3 * i] = h[i].x;
        pts[3 * i + 1] = h[i].y;
        pts[3 * i + 2] = (float)h[i].status;
    }
}

void Tracker::update(int slot, const float* keypoints, const int* people, int nframes, int parts,
                     int64_t* ids_out)
{
    OPK_CHECK_ARG(slot == 0 || slot == 1, "slot 0 or 1");
    OPK_CHECK_ARG(nframes >= 0 && parts > 0, "negative frame count or no parts");
    if (nframes == 0) return;
    OPK_CHECK_ARG(people != nullptr, "NULL people counts");
    if (slot_n_[slot] != nframes)
        throw Error(3, "the slot's pyramid holds " + std::to_string(slot_n_[slot]) + " frames, not " +
                           std::to_string(nframes));
    if (has_prev_ && parts != parts_)
        throw Error(3, "the tracker holds people of another part count: reset it first");
    std::vector<size_t> first(nframes + 1, 0);
    for (int f = 0; f < nframes; ++f) {
        OPK_CHECK_ARG(people[f] >= 0, "negative people count");
        first[f + 1] = first[f] + (size_t)people[f];
    }
    OPK_CHECK_ARG(first[nframes] == 0 || (keypoints && ids_out), "NULL keypoints or ids");
    ctx_->bind();
    parts_ = parts;
    const size_t person = (size_t)parts * 3;
    double waited = 0.;
    const auto t0 = std::chrono::steady_clock::now();

    // 1. capture: (x, y, status), status 1 below the confidence
    std::vector<float> capture(first[nframes] * person);
    for (size_t i = 0; i < first[nframes] * (size_t)parts; ++i) {
        capture[3 * i] = keypoints[3 * i];
        capture[3 * i + 1] = keypoints[3 * i + 1];
        capture[3 * i + 2] = keypoints[3 * i + 2] < confidence_ ? 1.f : 0.f;
    }

    // 2. the fresh points of the whole batch in one launch: what frame f - 1 detected, into frame f
    //    (frame -1: the carried-in frame and its people)
    const size_t carried = has_prev_ ? last_capture_.size() / 3 : 0;
    std::vector<size_t> fresh_at(nframes + 1, 0);   // first fresh point of the people going INTO frame f
    fresh_at[0] = 0;
    for (int f = 0; f < nframes; ++f)
        fresh_at[f + 1] = fresh_at[f] + (f == 0 ? carried : (size_t)people[f - 1] * parts);
    std::vector<float> fresh(fresh_at[nframes] * 3);
    std::vector<int> fi(fresh_at[nframes]), fj(fresh_at[nframes]);
    for (int f = 0; f < nframes; ++f) {
        const size_t count = fresh_at[f + 1] - fresh_at[f];
        if (count == 0) continue;
        const float* src = f == 0 ? last_capture_.data() : capture.data() + first[f - 1] * person;
        std::memcpy(fresh.data() + fresh_at[f] * 3, src, count * 3 * sizeof(float));
        std::fill(fi.begin() + (long)fresh_at[f], fi.begin() + (long)fresh_at[f + 1], f - 1);
        std::fill(fj.begin() + (long)fresh_at[f], fj.begin() + (long)fresh_at[f + 1], f);
    }
    {
        const auto tw = std::chrono::steady_clock::now();
        propagate(slot, fresh.data(), fresh_at[nframes], fi.data(), fj.data());
        waited += ms_since(tw);
    }

    // 3. the frames in order
    std::vector<float> stale, flat;
    std::vector<int> si, sj;
    std::vector<Entry*> stale_of;
    std::vector<int64_t> ids;
    for (int f = 0; f < nframes; ++f) {
        const int np = people[f];
        const float* cap = capture.data() + first[f] * person;
        if (!has_prev_ && f == 0) {
            // initializeLK: every person becomes an entry
            for (int i = 0; i < np; ++i) {
                Entry& e = entries_[next_id_++];
                e.pts.assign(cap + i * person, cap + (i + 1) * person);
                e.counter = 0;
                e.src = i;
            }
        } else {
            // updateLK: age, erase, propagate
            stale.clear();
            stale_of.clear();
            for (auto it = entries_.begin(); it != entries_.end();) {
                Entry& e = it->second;
                if (e.counter++ > frames_to_delete_) {
                    it = entries_.erase(it);
                    continue;
                }
                if (e.counter == 1) {   // taken from the frame before: its points went ahead
                    const float* r = fresh.data() + (fresh_at[f] + (size_t)e.src * parts) * 3;
                    e.pts.assign(r, r + person);
                } else {
                    stale_of.push_back(&e);
                    stale.insert(stale.end(), e.pts.begin(), e.pts.end());
                }
                ++it;
            }
            if (!stale_of.empty()) {
                si.assign(stale.size() / 3, f - 1);
                sj.assign(stale.size() / 3, f);
                const auto tw = std::chrono::steady_clock::now();
                propagate(slot, stale.data(), stale.size() / 3, si.data(), sj.data());
                waited += ms_since(tw);
                for (size_t k = 0; k < stale_of.size(); ++k)
                    stale_of[k]->pts.assign(stale.begin() + (long)(k * person),
                                            stale.begin() + (long)((k + 1) * person));
            }
        }
        // matchLKAndOPGreedy
        flat.clear();
        ids.clear();
        for (const auto& kv : entries_) {
            ids.push_back(kv.first);
            flat.insert(flat.end(), kv.second.pts.begin(), kv.second.pts.end());
        }
        int64_t* out = ids_out + first[f];
        match_people(flat.data(), ids.data(), (int)ids.size(), cap, np, parts, inlier_ratio_,
                     distance_, layout_.w[0], layout_.h[0], &next_id_, out);
        for (int i = 0; i < np; ++i) {
            Entry& e = entries_[out[i]];
            e.pts.assign(cap + i * person, cap + (i + 1) * person);
            e.counter = 0;
            e.src = i;
        }
    }

    // 4. what the next call starts from: the last frame's pyramid and people
    const uint8_t* last = static_cast<const uint8_t*>(pyr_[slot].ptr) + (size_t)(nframes - 1) * layout_.frame;
    OPK_HIP(hipMemcpyAsync(carry_.get(layout_.frame), last, layout_.frame, hipMemcpyDeviceToDevice,
                           ctx_->stream));
    last_capture_.assign(capture.begin() + (long)(first[nframes - 1] * person), capture.end());
    has_prev_ = true;
    slot_n_[slot] = 0;
    ++batches_;
    host_ms_ += ms_since(t0) - waited;
}

}  // namespace opk
