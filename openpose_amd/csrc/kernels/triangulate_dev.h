// triangulate_dev.h -- one 3-D point from its views, as include/opk.h states it ("3-D keypoints
// from a camera rig"): validity, the 2V x 4 matrix, the one-sided Jacobi null vector, the
// reprojection error, the leave-one-out step and an array's acceptance.  Compiles for host and
// device: opk_triangulate_host (host/triangulate.cpp) and the kernels (triangulate.hip) run this
// very text, so with -ffp-contract=off both round every operation alike.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>

#if defined(__HIP__)
#define OPK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define OPK_HD inline
#endif

namespace opk {

constexpr int kTriMaxViews = 7;
constexpr int kTriRows = 2 * kTriMaxViews;

// the checked rig (host/triangulate.cpp: make_rig); passed to the kernels by value
struct TriRig {
    int views = 0;
    int min_views = 0;    // the effective value
    double max_acc = 0.;  // 25*sqrt(w0*h0/1310720.)
    double P[kTriMaxViews][12] = {};   // views past `views`: zeros, never used
    int w[kTriMaxViews] = {}, h[kTriMaxViews] = {};
};

struct TriSolve {
    double x, y, z, err;
};
struct TriPoint {
    double x, y, z, err;
    int dropped;
};

// the valid views of one part of one step (isValidKeypoint): their mask and count, and their
// (x, y) as doubles.  kp: the step's [V][parts][3]; present: its [V]
OPK_HD unsigned tri_gather(const TriRig& rig, const float* kp, const int* present, int parts,
                           int part, double (&xs)[kTriMaxViews], double (&ys)[kTriMaxViews],
                           int& nvalid)
{
    unsigned mask = 0;
    nvalid = 0;
#pragma unroll
    for (int i = 0; i < kTriMaxViews; ++i) {
        xs[i] = 0.;
        ys[i] = 0.;
        if (i < rig.views && present[i] != 0) {
            const float* k = kp + ((size_t)i * parts + part) * 3;
            const float x = k[0], y = k[1], s = k[2];
            if (s > 0.35f && x > 8.f && x < (float)(rig.w[i] - 8) && y > 8.f &&
                y < (float)(rig.h[i] - 8)) {
                mask |= 1u << i;
                xs[i] = (double)x;
                ys[i] = (double)y;
                ++nvalid;
            }
        }
    }
    return mask;
}

// one Jacobi rotation of the columns I, J (false: the pair was skipped)
template <int I, int J>
OPK_HD bool tri_rotate(double (&A)[kTriRows][4], double (&V)[4][4], double (&W)[4])
{
    double p = 0.;
#pragma unroll
    for (int k = 0; k < kTriRows; ++k) p = p + A[k][I] * A[k][J];
    if (fabs(p) <= DBL_EPSILON * sqrt(W[I] * W[J])) return false;
    p = p * 2.;
    const double beta = W[I] - W[J];
    const double gamma = sqrt(p * p + beta * beta);
    double c, s;
    if (beta < 0.) {
        const double delta = (gamma - beta) * 0.5;
        s = sqrt(delta / gamma);
        c = p / (gamma * s * 2.);
    } else {
        c = sqrt((gamma + beta) / (gamma * 2.));
        s = p / (gamma * c * 2.);
    }
    double wi = 0., wj = 0.;
#pragma unroll
    for (int k = 0; k < kTriRows; ++k) {
        const double t0 = c * A[k][I] + s * A[k][J];
        const double t1 = c * A[k][J] - s * A[k][I];
        A[k][I] = t0;
        A[k][J] = t1;
        wi = wi + t0 * t0;
        wj = wj + t1 * t1;
    }
    W[I] = wi;
    W[J] = wj;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t0 = c * V[k][I] + s * V[k][J];
        const double t1 = c * V[k][J] - s * V[k][I];
        V[k][I] = t0;
        V[k][J] = t1;
    }
    return true;
}

// ONE TRIANGULATION over the views of `mask`
OPK_HD TriSolve tri_solve(const TriRig& rig, const double (&xs)[kTriMaxViews],
                          const double (&ys)[kTriMaxViews], unsigned mask)
{
    double A[kTriRows][4];
#pragma unroll
    for (int i = 0; i < kTriMaxViews; ++i) {
        const bool in = ((mask >> i) & 1u) != 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            A[2 * i][k] = in ? xs[i] * rig.P[i][8 + k] - rig.P[i][k] : 0.;
            A[2 * i + 1][k] = in ? ys[i] * rig.P[i][8 + k] - rig.P[i][4 + k] : 0.;
        }
    }
    double V[4][4], W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double w = 0.;
#pragma unroll
        for (int k = 0; k < kTriRows; ++k) w = w + A[k][i] * A[k][i];
        W[i] = w;
#pragma unroll
        for (int k = 0; k < 4; ++k) V[k][i] = k == i ? 1. : 0.;
    }
#pragma nounroll
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool changed = tri_rotate<0, 1>(A, V, W);
        changed |= tri_rotate<0, 2>(A, V, W);
        changed |= tri_rotate<0, 3>(A, V, W);
        changed |= tri_rotate<1, 2>(A, V, W);
        changed |= tri_rotate<1, 3>(A, V, W);
        changed |= tri_rotate<2, 3>(A, V, W);
        if (!changed) break;
    }
    int m = 0;
    double wm = W[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (W[i] < wm) {
            wm = W[i];
            m = i;
        }
    double X[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = m == 0 ? V[k][0] : m == 1 ? V[k][1] : m == 2 ? V[k][2] : V[k][3];
    const double v3 = X[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = X[k] / v3;
    double sum = 0.;
    int count = 0;
#pragma unroll
    for (int i = 0; i < kTriMaxViews; ++i) {
        if (((mask >> i) & 1u) == 0) continue;
        double r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double a = 0.;
#pragma unroll
            for (int k = 0; k < 4; ++k) a = a + rig.P[i][4 * j + k] * X[k];
            r[j] = a;
        }
        const double dx = r[0] / r[2] - xs[i];
        const double dy = r[1] / r[2] - ys[i];
        sum = sum + sqrt(dx * dx + dy * dy);
        ++count;
    }
    return TriSolve{X[0], X[1], X[2], sum / (double)count};
}

// ONE POINT, the sequential statement: all valid views, then the leave-one-out step
OPK_HD TriPoint tri_point(const TriRig& rig, const double (&xs)[kTriMaxViews],
                          const double (&ys)[kTriMaxViews], unsigned mask, int nvalid)
{
    const TriSolve full = tri_solve(rig, xs, ys, mask);
    TriPoint out{full.x, full.y, full.z, full.err, -1};
    if (nvalid >= 4 && full.err > 0.5 * rig.max_acc) {
        double best = full.err;
#pragma nounroll
        for (int i = 0; i < kTriMaxViews; ++i) {
            if (((mask >> i) & 1u) == 0) continue;
            const TriSolve sub = tri_solve(rig, xs, ys, mask & ~(1u << i));
            if (best > sub.err && sub.err < 0.9 * full.err) {
                best = sub.err;
                out = TriPoint{sub.x, sub.y, sub.z, sub.err, i};
            }
        }
    }
    return out;
}

OPK_HD bool tri_finite(float v) { return fabsf(v) <= FLT_MAX; }

// ONE ARRAY OF A STEP: xyz [parts][4] holds each attempted part's three floats (anything in
// [3]), err [parts] its error or -1; on return xyz is the step's result.  Returns the status.
OPK_HD int tri_accept(const TriRig& rig, int parts, float* xyz, const double* err)
{
    double sum = 0.;
    int count = 0;
    for (int p = 0; p < parts; ++p)
        if (err[p] != -1.) {
            sum = sum + err[p];
            ++count;
        }
    const double total = count > 0 ? sum / (double)count : 0.;
    for (int p = 0; p < parts; ++p) {
        float* o = xyz + (size_t)p * 4;
        const double e = err[p];
        const bool keep = count > 0 && e != -1. && tri_finite(o[0]) && tri_finite(o[1]) &&
                          tri_finite(o[2]) && e < 5 * total && e < rig.max_acc;
        if (keep) {
            o[3] = 1.f;
        } else {
            o[0] = 0.f;
            o[1] = 0.f;
            o[2] = 0.f;
            o[3] = 0.f;
        }
    }
    return count > 0 ? 1 : 0;
}

}  // namespace opk
