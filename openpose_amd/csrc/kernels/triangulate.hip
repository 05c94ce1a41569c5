// triangulate.hip -- 3-D keypoints from a camera rig (op::PoseTriangulation::reconstructArray,
// --3d) for every point of a batch in one launch.  include/opk.h ("3-D keypoints from a camera
// rig") is the definition; the arithmetic of a point is triangulate_dev.h, the text the host route
// runs too.
//
// A point is one triangulation over its valid views and, when it sits badly, one more without each
// of them: up to 8 independent Jacobi solves of a 14 x 4 matrix.  Two mappings are built and held
// to the host route bit for bit:
//   triangulate<group>   8 lanes per point, 8 points per wave (shipped): lane 0 of a group solves
//                        over all valid views, lane s without view s-1; the subsets are solved
//                        whether or not the leave-one-out step applies -- the lanes would idle
//                        otherwise -- and the choice among them is a shuffle minimum over
//                        (error, lane), which is the sequential rule's choice: the first of the
//                        smallest errors below 0.9 e;
//   triangulate<thread>  a thread per point running the sequential statement (dev switch
//                        TRI_GROUP=0): a lane whose point needs the leave-one-out step holds its
//                        whole wave for up to 8 solves one after the other.
// Both keep the matrix, V and W in registers: every loop over rows and columns has a fixed trip
// count and is unrolled, the views a set goes without are zero rows.  The times of both are in
// profiles/triangulate/README.md.
// The acceptance of an array needs the mean of its errors summed in part order: a second launch,
// one lane per array, walks its <= 70 parts.
#include "triangulate_dev.h"

#include "../common.h"
#include "../host/context.h"
#include "../host/triangulate.h"

namespace opk {

namespace {

constexpr int kGroup = 8;                 // lanes per point
constexpr int kPointsPerWave = 64 / kGroup;

// grid ceil(points / 8), block 64.  kp [steps][V][parts][3], present [steps][V]; writes of every
// point: xyz [steps][parts][4] (the three floats of an attempted part, else zeros), err
// [steps][parts] (-1: not attempted), dropped [steps][parts] (may be NULL)
__global__ __launch_bounds__(64) void triangulate_group_kernel(TriRig rig, const float* __restrict__ kp,
                                                               const int* __restrict__ present,
                                                               int parts, int npoints,
                                                               float* __restrict__ xyz,
                                                               double* __restrict__ err,
                                                               int* __restrict__ dropped)
{
    const int lane = (int)threadIdx.x, sub = lane & (kGroup - 1), lead = lane & ~(kGroup - 1);
    int p = (int)blockIdx.x * kPointsPerWave + (lane >> 3);
    const bool live = p < npoints;
    if (!live) p = npoints - 1;   // the lanes past the end redo the last point and write nothing
    const int t = p / parts, part = p - t * parts;
    double xs[kTriMaxViews], ys[kTriMaxViews];
    int nvalid;
    const unsigned mask = tri_gather(rig, kp + (size_t)t * rig.views * parts * 3,
                                     present + (size_t)t * rig.views, parts, part, xs, ys, nvalid);
    const bool attempted = nvalid >= rig.min_views;
    // lane s > 0: the set without view s-1, if that is a valid view and the step can apply
    const bool subset = sub > 0 && attempted && nvalid >= 4 && ((mask >> (sub - 1)) & 1u) != 0;
    TriSolve r{0., 0., 0., 0.};
    if (attempted && (sub == 0 || subset))
        r = tri_solve(rig, xs, ys, sub == 0 ? mask : mask & ~(1u << (sub - 1)));
    const double e = __shfl(r.err, lead);
    const bool cand = subset && e > 0.5 * rig.max_acc && r.err < 0.9 * e;
    // the first of the smallest candidate errors; no candidate: lane 0, the full set
    double key = cand ? r.err : HUGE_VAL;
    int who = cand ? sub : 0;
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) {
        const double k2 = __shfl_xor(key, d);
        const int w2 = __shfl_xor(who, d);
        if (k2 < key || (k2 == key && w2 < who)) {
            key = k2;
            who = w2;
        }
    }
    const float x = (float)__shfl(r.x, lead + who);
    const float y = (float)__shfl(r.y, lead + who);
    const float z = (float)__shfl(r.z, lead + who);
    const double ew = __shfl(r.err, lead + who);
    if (live && sub == 0) {
        float* o = xyz + (size_t)p * 4;
        o[0] = attempted ? x : 0.f;
        o[1] = attempted ? y : 0.f;
        o[2] = attempted ? z : 0.f;
        o[3] = 0.f;
        err[p] = attempted ? ew : -1.;
        if (dropped) dropped[p] = attempted && who > 0 ? who - 1 : -1;
    }
}

// grid ceil(points / 64), block 64: a thread per point, the sequential statement
__global__ __launch_bounds__(64) void triangulate_thread_kernel(TriRig rig, const float* __restrict__ kp,
                                                                const int* __restrict__ present,
                                                                int parts, int npoints,
                                                                float* __restrict__ xyz,
                                                                double* __restrict__ err,
                                                                int* __restrict__ dropped)
{
    const int p = (int)(blockIdx.x * 64 + threadIdx.x);
    if (p >= npoints) return;
    const int t = p / parts, part = p - t * parts;
    double xs[kTriMaxViews], ys[kTriMaxViews];
    int nvalid;
    const unsigned mask = tri_gather(rig, kp + (size_t)t * rig.views * parts * 3,
                                     present + (size_t)t * rig.views, parts, part, xs, ys, nvalid);
    float x = 0.f, y = 0.f, z = 0.f;
    double e = -1.;
    int d = -1;
    if (nvalid >= rig.min_views) {
        const TriPoint r = tri_point(rig, xs, ys, mask, nvalid);
        x = (float)r.x;
        y = (float)r.y;
        z = (float)r.z;
        e = r.err;
        d = r.dropped;
    }
    float* o = xyz + (size_t)p * 4;
    o[0] = x;
    o[1] = y;
    o[2] = z;
    o[3] = 0.f;
    err[p] = e;
    if (dropped) dropped[p] = d;
}

// grid ceil(steps / 64), block 64: a lane per array
__global__ __launch_bounds__(64) void triangulate_accept_kernel(TriRig rig, int steps, int parts,
                                                                float* __restrict__ xyz,
                                                                const double* __restrict__ err,
                                                                int* __restrict__ status)
{
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= steps) return;
    status[t] = tri_accept(rig, parts, xyz + (size_t)t * parts * 4, err + (size_t)t * parts);
}

}  // namespace

void launch_triangulate(const TriRig& rig, int steps, int parts, const float* kp, const int* present,
                        float* xyz, int* status, double* err, int* dropped, hipStream_t stream)
{
    OPK_CHECK_ARG(steps >= 0 && parts > 0 && (long long)steps * parts <= (1 << 28),
                  "bad steps or parts");
    if (steps == 0) return;
    OPK_CHECK_ARG(kp && present && xyz && status && err, "NULL argument");
    const int npoints = steps * parts;
    if (dev_switch("TRI_GROUP", 1) != 0) {
        note_launch("triangulate<group>");
        hipLaunchKernelGGL(triangulate_group_kernel,
                           dim3((unsigned)((npoints + kPointsPerWave - 1) / kPointsPerWave)), dim3(64),
                           0, stream, rig, kp, present, parts, npoints, xyz, err, dropped);
    } else {
        note_launch("triangulate<thread>");
        hipLaunchKernelGGL(triangulate_thread_kernel, dim3((unsigned)((npoints + 63) / 64)), dim3(64),
                           0, stream, rig, kp, present, parts, npoints, xyz, err, dropped);
    }
    OPK_LAUNCH_CHECK();
    hipLaunchKernelGGL(triangulate_accept_kernel, dim3((unsigned)((steps + 63) / 64)), dim3(64), 0,
                       stream, rig, steps, parts, xyz, err, status);
    OPK_LAUNCH_CHECK();
}

// opk_triangulate: the two launches on the context's stream; errors NULL: the context's scratch
void triangulate(Context* ctx, const TriRig& rig, int steps, int parts, const float* kp,
                 const int* present, float* xyz, int* status, double* errors, int* dropped)
{
    OPK_CHECK_ARG(steps >= 0 && parts > 0, "bad steps or parts");
    if (steps == 0) return;
    ctx->bind();
    if (!errors)
        errors = static_cast<double*>(ctx->tri_errors.get((size_t)steps * parts * sizeof(double)));
    launch_triangulate(rig, steps, parts, kp, present, xyz, status, errors, dropped, ctx->stream);
}

}  // namespace opk
