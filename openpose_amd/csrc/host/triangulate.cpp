// triangulate.cpp -- the host route of the 3-D reconstruction (include/opk.h): rig checks, the
// camera matrix product and opk_triangulate_host.  Pure host code: no context, no device call.
#include "triangulate.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../../include/opk.h"
#include "../common.h"

namespace opk {

TriRig make_rig(const ::opk_rig* rig)
{
    OPK_CHECK_ARG(rig != nullptr, "NULL rig");
    OPK_CHECK_ARG(rig->views >= 2,
                  "3-D reconstruction (`--3d`) requires at least 2 camera views, only found " +
                      std::to_string(rig->views) + " camera parameter matrices.");
    OPK_CHECK_ARG(rig->views <= kTriMaxViews, "at most 7 camera views (the reference refuses a "
                                              "point seen by 8 or more)");
    OPK_CHECK_ARG(rig->camera_matrices && rig->image_sizes, "NULL camera matrices or image sizes");
    OPK_CHECK_ARG(rig->min_views < 0 || rig->min_views >= 2,
                  "Minimum number of views must be at least 2 (e.g., `--3d_min_views 2`) or negative.");
    TriRig r;
    r.views = rig->views;
    r.min_views = rig->min_views > 0 ? rig->min_views : std::max(2, std::min(4, rig->views - 1));
    for (int v = 0; v < r.views; ++v) {
        for (int k = 0; k < 12; ++k) {
            const double e = rig->camera_matrices[v * 12 + k];
            OPK_CHECK_ARG(std::isfinite(e), "camera matrix entry is not finite");
            r.P[v][k] = e;
        }
        const int w = rig->image_sizes[2 * v], h = rig->image_sizes[2 * v + 1];
        OPK_CHECK_ARG(w > 0 && h > 0 && (long long)w * h <= INT_MAX, "bad image size");
        r.w[v] = w;
        r.h[v] = h;
    }
    r.max_acc = 25 * std::sqrt(r.w[0] * r.h[0] / 1310720.);
    return r;
}

void camera_matrix(const double* K, const double* Rt, double* out)
{
    OPK_CHECK_ARG(K && Rt && out, "NULL argument");
    double m[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.;
            for (int k = 0; k < 3; ++k) s = s + K[3 * i + k] * Rt[4 * k + j];
            m[4 * i + j] = s;
        }
    std::copy(m, m + 12, out);
}

void triangulate_host(const TriRig& rig, int steps, int parts, const float* kp, const int* present,
                      float* xyz, int* status, double* errors, int* dropped)
{
    OPK_CHECK_ARG(steps >= 0 && parts > 0, "bad steps or parts");
    if (steps == 0) return;
    OPK_CHECK_ARG(kp && present && xyz && status, "NULL argument");
    std::vector<double> err_own;
    if (!errors) err_own.resize((size_t)parts);
    for (int t = 0; t < steps; ++t) {
        const float* skp = kp + (size_t)t * rig.views * parts * 3;
        const int* spr = present + (size_t)t * rig.views;
        float* sx = xyz + (size_t)t * parts * 4;
        double* se = errors ? errors + (size_t)t * parts : err_own.data();
        for (int p = 0; p < parts; ++p) {
            double xs[kTriMaxViews], ys[kTriMaxViews];
            int nvalid = 0;
            const unsigned mask = tri_gather(rig, skp, spr, parts, p, xs, ys, nvalid);
            float* o = sx + (size_t)p * 4;
            o[0] = o[1] = o[2] = o[3] = 0.f;
            se[p] = -1.;
            if (dropped) dropped[(size_t)t * parts + p] = -1;
            if (nvalid < rig.min_views) continue;
            const TriPoint r = tri_point(rig, xs, ys, mask, nvalid);
            o[0] = (float)r.x;
            o[1] = (float)r.y;
            o[2] = (float)r.z;
            se[p] = r.err;
            if (dropped) dropped[(size_t)t * parts + p] = r.dropped;
        }
        status[t] = tri_accept(rig, parts, sx, se);
    }
}

}  // namespace opk

// (the entry points below keep a guard of their own: this file also links into a stand-alone
// program without api.cpp)
template <class F>
static int tri_guarded(F&& f)
{
    try {
        f();
        return OPK_OK;
    } catch (const opk::Error& e) {
        opk::set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        opk::set_error(e.what());
        return OPK_ERR_STATE;
    }
}

extern "C" {

int opk_camera_matrix(const double* intrinsics, const double* extrinsics, double* out)
{
    return tri_guarded([&] { opk::camera_matrix(intrinsics, extrinsics, out); });
}

int opk_triangulate_host(const opk_rig* rig, int steps, int parts, const float* keypoints_host,
                         const int* present_host, float* xyz_host, int* status_host,
                         double* errors_host, int* dropped_host)
{
    return tri_guarded([&] {
        const opk::TriRig r = opk::make_rig(rig);
        opk::triangulate_host(r, steps, parts, keypoints_host, present_host, xyz_host, status_host,
                              errors_host, dropped_host);
    });
}

}  // extern "C"
