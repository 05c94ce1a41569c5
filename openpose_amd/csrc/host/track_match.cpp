// track_match.cpp -- matchLKAndOPGreedy (src/openpose/tracking/personIdExtractor.cpp:168-290) as a
// pure host function on arrays; the definition, tie rule included: include/opk.h.
#include <algorithm>
#include <cmath>
#include <vector>

#include "track.h"

namespace opk {

namespace {

struct Candidate {
    float total;
    int person, entry;   // entry: index into the ascending id list
};

// The order the round's candidates are taken in: the smallest total distance first (the reference
// sorts descending and pops from the back); equal totals by the lower entry id, then the lower
// person index.  A NaN total comes after every number, so this is a strict weak order.
bool taken_before(const Candidate& a, const Candidate& b)
{
    const bool an = std::isnan(a.total), bn = std::isnan(b.total);
    if (an != bn) return bn;
    if (!an && a.total != b.total) return a.total < b.total;
    if (a.entry != b.entry) return a.entry < b.entry;
    return a.person < b.person;
}

}  // namespace

void match_people(const float* entries, const int64_t* entry_ids, int n_entries, const float* people,
                  int n_people, int parts, float inlier_ratio, float distance, int width, int height,
                  int64_t* next_id, int64_t* ids_out)
{
    OPK_CHECK_ARG(n_entries >= 0 && n_people >= 0 && parts > 0, "negative count or no parts");
    OPK_CHECK_ARG(next_id != nullptr, "NULL next_id");
    OPK_CHECK_ARG(n_entries == 0 || (entries && entry_ids), "NULL entries");
    OPK_CHECK_ARG(n_people == 0 || (people && ids_out), "NULL people");
    OPK_CHECK_ARG(width > 0 && height > 0, "empty frame");
    for (int e = 1; e < n_entries; ++e)
        OPK_CHECK_ARG(entry_ids[e - 1] < entry_ids[e], "entry ids must be strictly ascending");
    const size_t stride = (size_t)parts * 3;
    // fastMax(10.f, distanceThreshold * float(std::sqrt(cols * rows)) / 960.f)
    const float root = (float)std::sqrt((double)((long long)width * height));
    const float scaled = distance * root / 960.f;
    const float threshold = 10.f > scaled ? 10.f : scaled;

    std::vector<int> assigned(n_people, -1);   // entry index
    std::vector<char> used(n_entries, 0);
    std::vector<Candidate> candidates;
    bool converged = false;
    while (n_people > 0 && !converged) {
        candidates.clear();
        float best = 0.f;
        converged = true;
        for (int i = 0; i < n_people; ++i) {
            if (assigned[i] != -1) continue;
            const float* p = people + i * stride;
            for (int e = 0; e < n_entries; ++e) {
                if (used[e]) continue;
                const float* q = entries + e * stride;
                int inliers = 0, active = 0;
                float total = 0.f;
                for (int k = 0; k < parts; ++k) {
                    if (q[3 * k + 2] != 0.f || p[3 * k + 2] != 0.f) continue;
                    ++active;
                    const float dx = q[3 * k] - p[3 * k], dy = q[3 * k + 1] - p[3 * k + 1];
                    const float d = std::sqrt(dx * dx + dy * dy);
                    total += d;
                    if (d < threshold) ++inliers;
                }
                if (active == 0) continue;
                const float score = (float)inliers / (float)active;
                if (score == best && score >= inlier_ratio) {
                    candidates.push_back(Candidate{total, i, e});
                } else if (score > best && score >= inlier_ratio) {
                    best = score;
                    candidates.clear();
                    candidates.push_back(Candidate{total, i, e});
                }
            }
        }
        std::sort(candidates.begin(), candidates.end(), taken_before);
        for (const Candidate& c : candidates) {
            if (used[c.entry]) continue;
            assigned[c.person] = c.entry;   // (a person taken twice in a round keeps the later entry)
            used[c.entry] = 1;
            converged = false;
        }
    }
    for (int i = 0; i < n_people; ++i)
        ids_out[i] = assigned[i] != -1 ? entry_ids[assigned[i]] : (*next_id)++;
}

}  // namespace opk
