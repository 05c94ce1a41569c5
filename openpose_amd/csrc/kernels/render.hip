// render.hip -- the GPU renderers of pose / face / hand keypoints and of heat maps, on gfx950.
//
// Keypoints: renderKeypointsOld / renderKeypoints (include/openpose_private/utilities/render.hu:61-383)
// as launched by renderPoseKeypointsGpu (src/openpose/pose/renderPose.cu:609-748),
// renderFaceKeypointsGpu (src/openpose/face/renderFace.cu:48-76) and renderHandKeypointsGpu
// (src/openpose/hand/renderHand.cu:48-76).  The reference evaluates, for every pixel of the frame,
// each person's box test and every limb's atan2f / sinf / cosf.  Here:
//   1. render_prep_kernel (one wave per person): the person's box and scale
//      (getBoundingBoxPerPerson, render.hu:6-59) and, per limb and per part, everything that does not
//      depend on the pixel -- limb centre, cos / sin of its angle, the ellipse's aSqrt / bSqrt, the
//      circle radii -- with the reference's expressions, in its operation order;
//   2. render_keypoints_kernel (one 32x8 pixel tile per workgroup): the people whose box meets the
//      tile are compacted in order into LDS (wave ballots); then, in rounds of 256, their limbs and
//      part circles -- person-major, limbs before circles, the reference's draw order -- are culled
//      against the tile (a limb survives if the tile reaches its squared-distance bound
//      1.01 * (aSqrt + bSqrt) + 4, beyond which the ellipse test cannot pass since
//      judge >= dist^2 / (aSqrt + bSqrt); a circle if the tile reaches its radius) and the survivors'
//      records staged in LDS; each pixel then runs the reference's per-pixel tests on those only and
//      blends with addColorWeighted (cuda.hu:188-201).
// The frame is the reference's float BGR [h][w][3]; each pixel is read and written once: the
// kernel is bound by those 24 bytes per pixel (HBM) plus the per-person ALU work.
//
// Heat maps: renderBodyPartHeatMap (bicubic + getColorHeatMap), renderBodyPartHeatMaps (nearest,
// COCO colors) and renderPartAffinities (getColorXYAffinity) of renderPose.cu:44-119,419-527,
// one pixel per lane; the same arithmetic is the heat layer of the fused batch render
// (render_frames_kernel), there on heat values staged per tile in LDS or evaluated lazily.
//
// Arithmetic is the reference's expression by expression with every mul / add rounded separately
// (the library builds with -ffp-contract=off); atan2f / sinf / cosf are the device library's, so
// pixels on an ellipse boundary (|judge - 1| ~ 1e-6) and PAF colours (~1e-4 of 255) can differ
// from the CUDA build's: that part of render parity is unpinned.
#include "kernels.h"
#include "heat_dev.h"
#include "warp_dev.h"
#include "yuv_dev.h"
#include "yuv_out_dev.h"
#include "../common.h"
#include "../host/frames.h"

#include <cmath>

namespace opk {

namespace {

constexpr int kTileW = 32, kTileH = 8;
static_assert(kTileW == kYuvTileW && kTileH == kYuvTileH, "yuv_store_tile stages the render's tile");
// float(pi) as renderPose.cu:10's __constant__ PI rounds
constexpr float kPi = 3.14159265358979323846f;

// fastTruncateCuda (cuda.hu:84-88): fastMin(hi, fastMax(lo, v)) with its NaN behaviour
__device__ __forceinline__ float truncate_ref(float v, float lo, float hi)
{
    const float m = lo > v ? lo : v;
    return hi < m ? hi : m;
}

__device__ __forceinline__ void blend(float& r, float& g, float& b, float cr, float cg, float cb,
                                      float alpha)
{
    // addWeighted: (1 - alpha) * value1 + alpha * value2
    r = (1.f - alpha) * r + alpha * cr;
    g = (1.f - alpha) * g + alpha * cg;
    b = (1.f - alpha) * b + alpha * cb;
}

// one wave per person: box (a lane-strided scan + wave reduction; min / max do not depend on the
// order), then lanes take limbs and parts
__device__ __forceinline__ void render_prep_person(const RenderKeypointsArgs& a, int p, int lane)
{
    const float* kp = a.kp + (size_t)p * a.parts * 3;
    float* box = a.geom + (size_t)p * 8;
    float* limb = a.geom + (size_t)a.people * 8 + (size_t)p * a.npairs * 8;
    float* part = a.geom + (size_t)a.people * 8 + (size_t)a.people * a.npairs * 8 +
                  (size_t)p * a.parts * 8;
    // getBoundingBoxPerPerson (render.hu:6-59 / 219-260)
    float minx = (float)a.w, miny = (float)a.h, maxx = 0.f, maxy = 0.f;
    for (int i = lane; i < a.parts; i += 64) {
        const float x = kp[3 * i], y = kp[3 * i + 1], s = kp[3 * i + 2];
        if (s > a.threshold) {
            if (x < minx) minx = x;
            if (x > maxx) maxx = x;
            if (y < miny) miny = y;
            if (y > maxy) maxy = y;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float a0 = __shfl_xor(minx, o), a1 = __shfl_xor(miny, o);
        const float a2 = __shfl_xor(maxx, o), a3 = __shfl_xor(maxy, o);
        minx = a0 < minx ? a0 : minx;
        miny = a1 < miny ? a1 : miny;
        maxx = a2 > maxx ? a2 : maxx;
        maxy = a3 > maxy ? a3 : maxy;
    }
    // the box's own scale; the reference leaves it unset when a coordinate maximum is exactly 0
    // (then only the box test decides, which rejects every pixel of an empty person)
    const float scale = truncate_ref(((maxx - minx) + (maxy - miny)) / 400.f, 0.33f, 1.f);
    if (maxx != 0.f && maxy != 0.f) {
        maxx += 50.f;
        maxy += 50.f;
        minx -= 50.f;
        miny -= 50.f;
    }
    if (lane == 0) {
        box[0] = minx;
        box[1] = miny;
        box[2] = maxx;
        box[3] = maxy;
        box[4] = scale;
    }
    const float s2 = scale * scale;
    const float lw2 = a.line_width * a.line_width;
    const float r2 = a.radius * a.radius;
    // limbs (render.hu:288-326)
    for (int j = lane; j < a.npairs; j += 64) {
        const unsigned pa = a.pairs[2 * j], pb = a.pairs[2 * j + 1];
        const float xA = kp[3 * pa], yA = kp[3 * pa + 1], sA = kp[3 * pa + 2];
        const float xB = kp[3 * pb], yB = kp[3 * pb + 1], sB = kp[3 * pb + 2];
        float* L = limb + (size_t)j * 8;
        if (sA > a.threshold && sB > a.threshold) {
            const float k = a.scales[pb % a.nscales];
            const float ks = k * k * k;
            const float bSqrt = s2 * (lw2 * ks);
            const float xP = (xA + xB) / 2.f, yP = (yA + yB) / 2.f;
            const float aSqrt = (xA - xP) * (xA - xP) + (yA - yP) * (yA - yP);
            const float angle = atan2f(yB - yA, xB - xA);
            L[0] = xP;
            L[1] = yP;
            L[2] = cosf(angle);
            L[3] = sinf(angle);
            L[4] = aSqrt;
            L[5] = bSqrt;
            L[6] = 1.01f * (aSqrt + bSqrt) + 4.f;   // squared-distance bound of the ellipse
            L[7] = (float)((pb % a.ncolors) * 3);
        } else {
            L[6] = -1.f;   // a score at or below the threshold: never drawn
        }
    }
    // part circles (render.hu:329-377)
    for (int i = lane; i < a.parts; i += 64) {
        float* C = part + (size_t)i * 8;
        const float x = kp[3 * i], y = kp[3 * i + 1], s = kp[3 * i + 2];
        if (!(s > a.threshold)) {
            C[4] = 0.f;
            continue;
        }
        const float k = a.scales[i % a.nscales];
        const float radiusScaled = r2 * (k * k * k);
        C[0] = x;
        C[1] = y;
        if (i == a.eye1 || i == a.eye2) {
            const float eyeRatio = 2.5f * sqrtf(radiusScaled);
            C[2] = s2 * eyeRatio * eyeRatio;                  // maxr2
            C[3] = s2 * (eyeRatio - 2) * (eyeRatio - 2);      // minr2
            C[4] = 2.f;
        } else {
            C[2] = s2 * radiusScaled;
            C[3] = 0.f;
            C[4] = 1.f;
        }
        C[5] = (float)((i % a.ncolors) * 3);
    }
}

// a.people may span many frames (the batched render): a person's geometry does not depend on the
// frame, whose slice of people the draw kernel takes from the prefix offsets
__global__ __launch_bounds__(64) void render_prep_kernel(RenderKeypointsArgs a)
{
    render_prep_person(a, blockIdx.x, threadIdx.x);
}

// squared distance from (cx, cy) to the tile's pixel rectangle, with the per-pixel test's own
// operations at its nearest pixel: never above any pixel's dist^2 (rounding is monotonic)
__device__ __forceinline__ float rect_d2(float cx, float cy, float fx0, float fy0, float fx1,
                                         float fy1)
{
    const float dx = cx < fx0 ? fx0 - cx : (cx > fx1 ? cx - fx1 : 0.f);
    const float dy = cy < fy0 ? fy0 - cy : (cy > fy1 ? cy - fy1 : 0.f);
    return dx * dx + dy * dy;
}

// ordered compaction of one 256-candidate round: returns this thread's slot (or -1) and the
// round's total; wcount is the block's 4-entry scratch
__device__ __forceinline__ int compact(bool hit, int* wcount, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < 4; ++i) {
        off += i < wave ? wcount[i] : 0;
        tot += wcount[i];
    }
    *total = tot;
    return hit ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// One keypoint render's people as the draw stages see them: `people` consecutive persons of a
// geometry buffer (render_prep_person's layout), their colors and the blend weight.
struct RenderView {
    const float* boxes;     // [people][8]
    const float* limbs;     // [people][npairs][8]
    const float* circles;   // [people][parts][8]
    const float* colors;
    int people, npairs, parts;
    float alpha;
};
// `people` persons from person `first` of a geometry buffer that holds `total`
__device__ __forceinline__ RenderView render_view(const float* geom, int total, int first,
                                                  int people, int npairs, int parts,
                                                  const float* colors, float alpha)
{
    const float* limbs = geom + (size_t)total * 8;
    const float* circles = limbs + (size_t)total * npairs * 8;
    return RenderView{geom + (size_t)first * 8, limbs + (size_t)first * npairs * 8,
                      circles + (size_t)first * parts * 8, colors, people, npairs, parts, alpha};
}

// The workgroup's 32x8 pixel tile and this thread's pixel of it
struct RenderTile {
    float fx0, fy0, fx1, fy1;   // the tile's pixel rectangle, clipped to the frame
    int x, y;
    bool inside;
};
__device__ __forceinline__ RenderTile render_tile(int w, int h)
{
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    RenderTile t;
    t.fx0 = (float)tx0;
    t.fy0 = (float)ty0;
    t.fx1 = (float)min(tx0 + kTileW - 1, w - 1);
    t.fy1 = (float)min(ty0 + kTileH - 1, h - 1);
    t.x = tx0 + (threadIdx.x & (kTileW - 1));
    t.y = ty0 + threadIdx.x / kTileW;
    t.inside = t.x < w && t.y < h;
    return t;
}

// Stages 1 and 2 of the header comment for one view on the thread's pixel (b, g, r); every thread
// of the 256-thread workgroup calls it (barriers inside).  LDS: plist [kRenderMaxPeople], one
// round's drawable items in draw order -- {box}, {geometry}, {geometry, type, color} --, wcount [4].
__device__ __forceinline__ void render_view_pixel(const RenderView& a, const RenderTile& t,
                                                  unsigned short* plist, float4 (*items)[4],
                                                  int* wcount, float& b, float& g, float& r)
{
    const float fx0 = t.fx0, fy0 = t.fy0, fx1 = t.fx1, fy1 = t.fy1;
    const float* __restrict__ boxes = a.boxes;
    const float* __restrict__ limbs = a.limbs;
    const float* __restrict__ circles = a.circles;
    const float* __restrict__ colors = a.colors;

    // 1. the people whose box meets this tile, in person order
    int n = 0;
    for (int base = 0; base < a.people; base += 256) {
        const int p = base + threadIdx.x;
        bool hit = false;
        if (p < a.people) {
            const float* B = boxes + (size_t)p * 8;
            hit = B[2] >= fx0 && B[0] <= fx1 && B[3] >= fy0 && B[1] <= fy1;
        }
        int tot;
        const int slot = compact(hit, wcount, &tot);
        if (slot >= 0) plist[n + slot] = (unsigned short)p;
        __syncthreads();
        n += tot;
    }

    const int x = t.x;
    const bool inside = t.inside;
    const float fx = (float)t.x, fy = (float)t.y;

    // 2. rounds of 256 (person, limb | part) candidates, person-major, limbs before parts (the
    //    reference's draw order); those whose ellipse bound / circle reaches the tile go to LDS
    const int per = a.npairs + a.parts;
    const int total = n * per;
    for (int k0 = 0; k0 < total; k0 += 256) {
        const int k = k0 + threadIdx.x;
        bool hit = false;
        float4 q0, q1, q2, q3;
        if (k < total) {
            const int s = k / per, j = k - s * per;
            const int p = plist[s];
            const float* B = boxes + (size_t)p * 8;
            q0 = make_float4(B[0], B[1], B[2], B[3]);
            if (j < a.npairs) {
                const float* L = limbs + ((size_t)p * a.npairs + j) * 8;
                const float rej = L[6];
                if (rej >= 0.f || rej != rej) {
                    hit = !(rect_d2(L[0], L[1], fx0, fy0, fx1, fy1) > rej);
                    q1 = make_float4(L[0], L[1], L[2], L[3]);
                    q2 = make_float4(L[4], L[5], rej, L[7]);
                    q3 = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
                const float* C = circles + ((size_t)p * a.parts + (j - a.npairs)) * 8;
                const float kind = C[4];
                if (kind != 0.f) {
                    hit = !(rect_d2(C[0], C[1], fx0, fy0, fx1, fy1) > C[2]);
                    q1 = make_float4(C[0], C[1], C[2], C[3]);
                    q2 = make_float4(0.f, 0.f, 0.f, C[5]);
                    q3 = make_float4(kind, 0.f, 0.f, 0.f);
                }
            }
        }
        int m;
        const int slot = compact(hit, wcount, &m);
        if (slot >= 0) {
            items[slot][0] = q0;
            items[slot][1] = q1;
            items[slot][2] = q2;
            items[slot][3] = q3;
        }
        __syncthreads();
        if (inside) {
            for (int i = 0; i < m; ++i) {
                const float4 B = items[i][0];
                if (!(fx <= B.z && fx >= B.x && fy <= B.w && fy >= B.y)) continue;
                const float4 G = items[i][1], H = items[i][2];
                const float type = items[i][3].x;
                const float dx = fx - G.x, dy = fy - G.y;
                const float d2 = dx * dx + dy * dy;
                if (type == 0.f) {   // limb (render.hu:301-325)
                    if (d2 > H.z) continue;
                    const float A = G.z * dx + G.w * dy;
                    const float Bq = G.w * dx - G.z * dy;
                    const float judge = A * A / H.x + Bq * Bq / H.y;
                    if (0.f <= judge && judge <= 1.f) {
                        const float* c = colors + (int)H.w;
                        blend(r, g, b, c[0], c[1], c[2], a.alpha);
                    }
                } else if (type == 2.f) {   // googly eye (render.hu:344-366)
                    if (d2 <= G.z) {
                        float v = 0.f;
                        if (d2 <= G.w) v = 255.f;
                        if (d2 <= G.w * 0.6f) {
                            const float ex = (float)(x - 4) - G.x, ey = fy - G.y + 4;
                            if (ex * ex + ey * ey > 14.0625f) v = 0.f;
                        }
                        blend(r, g, b, v, v, v, 0.9f);
                    }
                } else if (0.f <= d2 && d2 <= G.z) {   // part circle (render.hu:368-375)
                    const float* c = colors + (int)H.w;
                    blend(r, g, b, c[0], c[1], c[2], a.alpha);
                }
            }
        }
        __syncthreads();   // the next round rewrites items
    }
}

__global__ __launch_bounds__(256) void render_keypoints_kernel(RenderKeypointsArgs a)
{
    __shared__ unsigned short plist[kRenderMaxPeople];
    __shared__ float4 items[256][4];
    __shared__ int wcount[4];
    const RenderTile t = render_tile(a.w, a.h);
    const size_t base = 3 * ((size_t)(t.inside ? t.y : 0) * a.w + (t.inside ? t.x : 0));
    float b = 0.f, g = 0.f, r = 0.f;
    if (t.inside && a.blend) {
        b = a.frame[base];
        g = a.frame[base + 1];
        r = a.frame[base + 2];
    }
    render_view_pixel(render_view(a.geom, a.people, 0, a.people, a.npairs, a.parts, a.colors,
                                  a.alpha),
                      t, plist, items, wcount, b, g, r);
    if (t.inside) {
        a.frame[base] = b;
        a.frame[base + 1] = g;
        a.frame[base + 2] = r;
    }
}

// ---- the output image: CvMatToOpOutput, OpOutputToCvMat and the fused batch render ---------------

// this thread's pixel of frame f as CvMatToOpOutput's warp (or copy, K == 0) gives it; Yuv: the
// frames are NV12 / I420 and every byte read is converted (yuv_dev.h), the copy included
template <int K, bool Yuv>
__device__ __forceinline__ void output_pixel(int u[3], const FrameWarp& wp, int f, int x, int y)
{
    const FrameSource& fs = wp.src;
    const uint8_t* fsrc = fs.plane[0] + (size_t)f * fs.frame[0];
    const size_t step = fs.step;
    // tap row yy: BGR bytes, or the luma and chroma rows
    auto row_of = [&](int, int yy) {
        if constexpr (Yuv) return yuv_row(fs, f, yy);
        else return fsrc + (size_t)yy * step;
    };
    if constexpr (K == 0) {
        warp_tap(u, row_of(0, y), x);
    } else {
        const int2 xt = reinterpret_cast<const int2*>(wp.xtab)[x];
        const int2 yt = reinterpret_cast<const int2*>(wp.ytab)[y];
        warp_pixel<K>(u, yt, xt, warp_weights<K>(wp.wtab, yt.y, xt.y), fs.h, fs.w, row_of);
    }
}

// OpOutputToCvMat's two casts of one value
__device__ __forceinline__ unsigned cast_u8(float v, int cast)
{
    if (cast == 0) {   // saturate_cast<uchar>(cvRound(v)): ties to even, then clamp
        const int i = __float2int_rn(v);
        return (unsigned)(i < 0 ? 0 : (i > 255 ? 255 : i));
    }
    return (unsigned)(int)truncate_ref(v, 0.f, 255.f);   // uCharImageCast (cuda.cu:27-34)
}

// one thread per output pixel, all three channels
template <int K, bool Yuv>
__global__ __launch_bounds__(256) void cvmat_to_output_kernel(float* __restrict__ dst, int w, int h,
                                                              FrameWarp wp)
{
    const RenderTile t = render_tile(w, h);
    if (!t.inside) return;
    int u[3];
    output_pixel<K, Yuv>(u, wp, blockIdx.z, t.x, t.y);
    float* o = dst + 3 * (((size_t)blockIdx.z * h + t.y) * w + t.x);
    o[0] = (float)u[0];
    o[1] = (float)u[1];
    o[2] = (float)u[2];
}

// rows of w*3 values; V: four values per thread (one 16-byte load, one 4-byte store) when every
// row of both arrays starts on such a boundary, else one value per thread
template <bool V>
__global__ __launch_bounds__(256) void output_to_cvmat_kernel(uint8_t* __restrict__ dst,
                                                              size_t dst_step,
                                                              const float* __restrict__ src,
                                                              int row_values, int h, int cast)
{
    const int i = (blockIdx.x * 256 + threadIdx.x) * (V ? 4 : 1);
    if (i >= row_values) return;   // V: row_values is a multiple of 4
    const size_t row = (size_t)blockIdx.z * h + blockIdx.y;
    const float* s = src + row * row_values + i;
    uint8_t* d = dst + row * dst_step + i;
    if (V) {
        const float4 v = *reinterpret_cast<const float4*>(s);
        *reinterpret_cast<unsigned*>(d) = cast_u8(v.x, cast) | cast_u8(v.y, cast) << 8 |
                                          cast_u8(v.z, cast) << 16 | cast_u8(v.w, cast) << 24;
    } else {
        *d = (uint8_t)cast_u8(*s, cast);
    }
}

// getColorHeatMap (renderPose.cu:44-80) with vmin 0, vmax 1
__device__ __forceinline__ void color_heat(float* c, float v)
{
    const float t = truncate_ref(v, 0.f, 1.f);
    if (t < 0.125f) {
        c[0] = 256.f * (0.5f + (t * 4.f));
        c[1] = 0.f;
        c[2] = 0.f;
    } else if (t < 0.375f) {
        c[0] = 255.f;
        c[1] = 256.f * (t - 0.125f) * 4.f;
        c[2] = 0.f;
    } else if (t < 0.625f) {
        c[0] = 256.f * (-4.f * t + 2.5f);
        c[1] = 255.f;
        c[2] = 256.f * (4.f * (t - 0.375f));
    } else if (t < 0.875f) {
        c[0] = 0.f;
        c[1] = 256.f * (-4.f * t + 3.5f);
        c[2] = 255.f;
    } else {
        c[0] = 0.f;
        c[1] = 0.f;
        c[2] = 256.f * (-4.f * t + 4.5f);
    }
}

// getColorAffinity (renderPose.cu:82-106) with vmin 0, vmax 1, then getColorXYAffinity's radius
__device__ __forceinline__ void color_xy_affinity(float* c, float x, float y)
{
    const float len = sqrtf(x * x + y * y);
    const float rad = 1.f < len ? 1.f : len;
    const float an = atan2f(-y, -x) / kPi;
    float fk = (an + 1.f) / 2.f;
    if (isnan(fk)) fk = 0.f;
    const float v = truncate_ref(fk, 0.f, 1.f) * 55;
    if (v < 15) {
        c[0] = 255.f; c[1] = 255.f * (v / 15); c[2] = 0.f;
    } else if (v < 15 + 6) {
        c[0] = 255.f * (1 - ((v - 15) / 6)); c[1] = 255.f; c[2] = 0.f;
    } else if (v < 15 + 6 + 4) {
        c[0] = 0.f * (1 - ((v - 15) / 6)); c[1] = 255.f; c[2] = 255.f * ((v - 15 - 6) / 4);
    } else if (v < 15 + 6 + 4 + 11) {
        c[0] = 0.f; c[1] = 255.f * (1 - ((v - 15 - 6 - 4) / 11)); c[2] = 255.f;
    } else if (v < 55 - 6) {
        c[0] = 255.f * ((v - 15 - 6 - 4 - 11) / 13); c[1] = 0.f; c[2] = 255.f;
    } else if (v < 55) {
        c[0] = 255.f; c[1] = 0.f; c[2] = 255.f * (1 - ((v - 15 - 6 - 4 - 11 - 13) / 6));
    } else {
        c[0] = 255.f; c[1] = 0.f; c[2] = 0.f;
    }
    c[0] *= rad;
    c[1] *= rad;
    c[2] *= rad;
}

__device__ __forceinline__ void blend_bgr(float* px, const float* c, float alpha)
{
    // addColorWeighted(target[+2], target[+1], target[+0], rgbColor, alpha)
    px[2] = (1.f - alpha) * px[2] + alpha * c[0];
    px[1] = (1.f - alpha) * px[1] + alpha * c[1];
    px[0] = (1.f - alpha) * px[0] + alpha * c[2];
}

// ---- the per-pixel arithmetic of the heat-map renders, shared by the per-frame kernels (which read
//      a materialised stack) and by the heat layer of render_frames_kernel (a staged window or a
//      lazy map).  A pixel first gathers its taps -- sample k of a HeatSampler around a base
//      (channel, x, y) --, then the functions below combine the gathered values.

// the heat-map coordinate a target pixel samples
__device__ __forceinline__ float heat_source(int x, float scale)
{
    return ((float)x + 0.5f) / scale - 0.5f;
}

// Tap k = 0 .. n-1 of a pixel: channel ch + (k >> cshift), column clamp(x + (k & xmask)), row
// clamp(y + ((k >> yshift) & ymask)), clamped into the map
struct HeatSampler {
    int n, cshift, xmask, yshift, ymask;
};
// cubicSequentialData's 4x4 taps (cuda.hu:92-109) from base (x1 - 1, y1 - 1): columns max(0, x1 - 1),
// x1, min(w - 1, x1 + 1), min(w - 1, min(w - 1, x1 + 1) + 1) are clamp(x1 - 1 + i) for x1 in the map
constexpr HeatSampler kSampleBicubic{16, 4, 3, 2, 3};
// one PAF bilinear: channel x then y, each (x1, y1), (x2, y1), (x1, y2), (x2, y2)
constexpr HeatSampler kSamplePaf{8, 2, 1, 1, 1};
// one PAF at its base pixel: channel x, channel y
constexpr HeatSampler kSamplePafBase{2, 0, 0, 0, 0};
constexpr HeatSampler kSampleOne{1, 0, 0, 0, 0};
constexpr int kHeatMaxTaps = 16;

struct HeatTap {
    int ch, x, y;
};
__device__ __forceinline__ HeatTap heat_tap(const HeatSampler& S, int k, int ch, int x, int y, int hw,
                                            int hh)
{
    return HeatTap{ch + (k >> S.cshift), heat_clampi(x + (k & S.xmask), 0, hw - 1),
                   heat_clampi(y + ((k >> S.yshift) & S.ymask), 0, hh - 1)};
}
// every tap from a materialised stack [channels][area]
__device__ __forceinline__ void heat_gather_stack(float* v, const HeatSampler& S,
                                                  const float* __restrict__ heat, size_t area, int ch,
                                                  int x, int y, int hw, int hh)
{
#pragma unroll
    for (int k = 0; k < kHeatMaxTaps; ++k)
        if (k < S.n) {
            const HeatTap t = heat_tap(S, k, ch, x, y, hw, hh);
            v[k] = heat[t.ch * area + (size_t)t.y * hw + t.x];
        }
}

// the base pixel and fractions of cubicSequentialData (bicubic and PAF samples)
struct HeatBase {
    int x1, y1;
    float dx, dy;
};
__device__ __forceinline__ HeatBase heat_base(float xs, float ys, int hw, int hh)
{
    HeatBase b;
    b.x1 = heat_clampi((int)floorf(xs), 0, hw - 1);
    b.dx = xs - (float)b.x1;
    b.y1 = heat_clampi((int)floorf(ys), 0, hh - 1);
    b.dy = ys - (float)b.y1;
    return b;
}

// renderBodyPartHeatMap (renderPose.cu:454-480): bicubicInterpolate (cuda.hu:125-145) of
// kSampleBicubic's values
__device__ __forceinline__ float heat_bicubic(const float* v, float dx, float dy)
{
    float t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = cuda_cubic(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], dx);
    return cuda_cubic(t[0], t[1], t[2], t[3], dy);
}

// renderBodyPartHeatMaps (renderPose.cu:419-452): the nearest sample's offset y * hw + x inside a
// plane.  int(xSource + 1e-5) is a double add, truncated into [0, width] (not width - 1), so the
// offset can pass the end of its row or plane by up to width + 1 values.
__device__ __forceinline__ size_t heat_maps_offset(float xs, float ys, int hw, int hh)
{
    int xh = (int)((double)xs + 1e-5), yh = (int)((double)ys + 1e-5);
    xh = xh > hw ? hw : (xh < 0 ? 0 : xh);
    yh = yh > hh ? hh : (yh < 0 ? 0 : yh);
    return (size_t)yh * hw + xh;
}
// one part's contribution: saturated value times the part's color
__device__ __forceinline__ void heat_maps_add(float* c, float h, const float* col)
{
    const float v = fminf(fmaxf(h, 0.f), 1.f);   // __saturatef (NaN -> 0)
    c[0] += v * col[0];
    c[1] += v * col[1];
    c[2] += v * col[2];
}

// renderPartAffinities (renderPose.cu:482-527): one PAF's color added to c; X / Y its gathered
// values: kSamplePaf's four each (bilinear) or the base pixel's
__device__ __forceinline__ void paf_add(float* c, const float* X, const float* Y, float dx, float dy,
                                        bool bilinear)
{
    float vx = X[0], vy = Y[0];
    if (bilinear) {
        const float xB = X[1], xC = X[2], xD = X[3];
        vx = (1 - dx) * (1 - dy) * vx + dx * (1 - dy) * xB + (1 - dx) * dy * xC + dx * dy * xD;
        const float yB = Y[1], yC = Y[2], yD = Y[3];
        vy = (1 - dx) * (1 - dy) * vy + dx * (1 - dy) * yB + (1 - dx) * dy * yC + dx * dy * yD;
    }
    float c2[3];
    color_xy_affinity(c2, vx, vy);
    c[0] += c2[0];
    c[1] += c2[1];
    c[2] += c2[2];
}

// renderBodyPartHeatMap: one channel, bicubic, getColorHeatMap
__global__ __launch_bounds__(256) void render_heat_map_kernel(RenderHeatArgs a, int part, int absv)
{
    const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= a.w || y >= a.h) return;
    const HeatBase hb = heat_base(heat_source(x, a.scale), heat_source(y, a.scale), a.hw, a.hh);
    float taps[kHeatMaxTaps];
    heat_gather_stack(taps, kSampleBicubic, a.heat, (size_t)a.hw * a.hh, part, hb.x1 - 1, hb.y1 - 1,
                      a.hw, a.hh);
    const float v = heat_bicubic(taps, hb.dx, hb.dy);
    float c[3];
    color_heat(c, absv ? fabsf(v) : v);
    blend_bgr(a.frame + 3 * ((size_t)y * a.w + x), c, a.alpha);
}

// renderBodyPartHeatMaps: every part, nearest sample, COCO colors
__global__ __launch_bounds__(256) void render_heat_maps_kernel(RenderHeatArgs a, int parts,
                                                               const float* __restrict__ colors,
                                                               int ncolors)
{
    const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= a.w || y >= a.h) return;
    const size_t off = heat_maps_offset(heat_source(x, a.scale), heat_source(y, a.scale), a.hw,
                                        a.hh);
    const size_t area = (size_t)a.hw * a.hh;
    // reads past the end of the last plane are clamped to the stack's last value
    const size_t last = area * parts - 1;
    float c[3] = {0.f, 0.f, 0.f};
    for (int p = 0; p < parts; ++p) {
        size_t idx = p * area + off;
        idx = idx > last ? last : idx;
        heat_maps_add(c, a.heat[idx], colors + (p % ncolors) * 3);
    }
    blend_bgr(a.frame + 3 * ((size_t)y * a.w + x), c, a.alpha);
}

// renderPartAffinities: `count` PAFs from channel `first`; one PAF is sampled bilinearly, several
// at the base pixel
__global__ __launch_bounds__(256) void render_pafs_kernel(RenderHeatArgs a, int first, int count)
{
    const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= a.w || y >= a.h) return;
    const HeatBase hb = heat_base(heat_source(x, a.scale), heat_source(y, a.scale), a.hw, a.hh);
    const size_t area = (size_t)a.hw * a.hh;
    const bool bilinear = count == 1;
    float c[3] = {0.f, 0.f, 0.f};
    for (int part = first; part < first + count * 2; part += 2) {
        float taps[kHeatMaxTaps];
        if (bilinear)
            heat_gather_stack(taps, kSamplePaf, a.heat, area, part, hb.x1, hb.y1, a.hw, a.hh);
        else
            heat_gather_stack(taps, kSamplePafBase, a.heat, area, part, hb.x1, hb.y1, a.hw, a.hh);
        paf_add(c, taps, taps + (bilinear ? 4 : 1), hb.dx, hb.dy, bilinear);
    }
    blend_bgr(a.frame + 3 * ((size_t)y * a.w + x), c, a.alpha);
}

// ---- the heat layer of the fused render ----------------------------------------------------------
// A 32x8 tile's pixels sample few heat pixels (about 20x8 per channel at scale 1.95), each of which
// a lazy map evaluates from 16 net-output taps.  The tile therefore evaluates the window of heat
// pixels it can touch once, cooperatively, into LDS (`win`, kRenderHeatWindow floats: the `items`
// array, idle before the keypoint layers), as many channels a pass as fit (all 25 parts of BODY_25
// at scale 1.95, its 52 PAF channels in two passes); the pixels gather from there.  A tap outside the staged window -- the flat-index overflow of the all-parts
// render, or every tap when the window does not fit (staged == 0: the heat map is much larger than
// the output) -- is evaluated directly by the same heat_at, so both routes give the same bits.
// heat_at is inlined at two places only, the staging loop and the loop over missed taps: each
// inlined copy reads the by-value kernel argument at some twenty places, and beyond a few hundred
// such reads the compiler copies the whole argument to scratch instead.
struct HeatWindow {
    const float* win;
    int x0, y0, w, h;    // the staged rectangle of heat pixels (w == 0: nothing staged)
    int plane0, planes;  // the staged channels
};

// the rectangle of base pixels clamp(floor(source)) of the tile, grown by lo / hi taps; staged
// only if `unit` channels of it fit
__device__ __forceinline__ HeatWindow heat_window(const RenderFramesHeat& H, const float* win, int lo,
                                                  int hi, int unit)
{
    HeatWindow W{win, 0, 0, 0, 0, 0, 0};
    if (!H.staged) return W;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    // the source coordinate does not decrease with the pixel: the tile's first and last pixel
    // bound every pixel's base
    const int bx0 = heat_clampi((int)floorf(heat_source(tx0, H.scale)), 0, H.map.w - 1);
    const int bx1 = heat_clampi((int)floorf(heat_source(tx0 + kTileW - 1, H.scale)), 0, H.map.w - 1);
    const int by0 = heat_clampi((int)floorf(heat_source(ty0, H.scale)), 0, H.map.h - 1);
    const int by1 = heat_clampi((int)floorf(heat_source(ty0 + kTileH - 1, H.scale)), 0, H.map.h - 1);
    const int x0 = max(0, bx0 - lo), x1 = min(H.map.w - 1, bx1 + hi);
    const int y0 = max(0, by0 - lo), y1 = min(H.map.h - 1, by1 + hi);
    const int w = x1 - x0 + 1, h = y1 - y0 + 1;
    // the launcher's bound holds for every tile; a window that did not fit would stay unstaged
    if (w <= 0 || h <= 0 || (long long)w * h * unit > kRenderHeatWindow) return W;
    W.x0 = x0;
    W.y0 = y0;
    W.w = w;
    W.h = h;
    return W;
}

// evaluate channels plane0 .. plane0 + planes - 1 of frame f over the window; every thread of the
// workgroup calls it (barriers inside when staging)
__device__ __forceinline__ void heat_stage(const RenderFramesHeat& H, HeatWindow& W, float* win, int f,
                                           int plane0, int planes)
{
    W.plane0 = plane0;
    W.planes = planes;
    if (!H.staged) return;
    __syncthreads();   // the previous pass's readers are done
    const int area = W.w * W.h, total = area * W.planes;
    for (int i = threadIdx.x; i < total; i += kTileW * kTileH) {
        const int p = i / area, r = i - p * area;
        const int y = r / W.w, x = r - y * W.w;
        win[i] = heat_at(H.map, f * H.map.channels + plane0 + p, W.x0 + x, W.y0 + y);
    }
    __syncthreads();
}

// the taps the staged window holds; returns the mask of those it does not
__device__ __forceinline__ unsigned heat_gather_window(float* v, const HeatSampler& S,
                                                       const HeatWindow& W, int ch, int x, int y,
                                                       int hw, int hh)
{
    unsigned miss = 0;
#pragma unroll
    for (int k = 0; k < kHeatMaxTaps; ++k)
        if (k < S.n) {
            const HeatTap t = heat_tap(S, k, ch, x, y, hw, hh);
            const unsigned wx = (unsigned)(t.x - W.x0), wy = (unsigned)(t.y - W.y0);
            const unsigned wp = (unsigned)(t.ch - W.plane0);
            if (wx < (unsigned)W.w && wy < (unsigned)W.h && wp < (unsigned)W.planes)
                v[k] = W.win[(wp * W.h + wy) * W.w + wx];
            else
                miss |= 1u << k;
        }
    return miss;
}
// the missed taps of frame f, evaluated
__device__ __forceinline__ void heat_gather_missed(float* v, unsigned miss, const HeatSampler& S,
                                                   const RenderFramesHeat& H, int f, int ch, int x,
                                                   int y)
{
#pragma unroll 1
    for (; miss; miss &= miss - 1) {
        const int k = __ffs(miss) - 1;
        const HeatTap t = heat_tap(S, k, ch, x, y, H.map.w, H.map.h);
        const float h = heat_at(H.map, f * H.map.channels + t.ch, t.x, t.y);
#pragma unroll
        for (int j = 0; j < kHeatMaxTaps; ++j) v[j] = j == k ? h : v[j];   // v stays in registers
    }
}

// the heat layer's kinds as the kernel is instantiated for them (each instantiation carries its own
// kind's code and registers only): bicubic part / distance, all parts, one or all PAFs
constexpr int kHeatModeNone = 0, kHeatModeCubic = 1, kHeatModeParts = 2, kHeatModePaf = 3;

// the heat layer on the thread's pixel (b, g, r) of frame f; every thread of the workgroup calls it
template <int Mode>
__device__ __forceinline__ void render_heat_pixel(const RenderFramesHeat& H, const RenderTile& t,
                                                  int f, float* win, float& b, float& g, float& r)
{
    const int hw = H.map.w, hh = H.map.h;
    const float xs = heat_source(t.x, H.scale), ys = heat_source(t.y, H.scale);
    constexpr bool cubic = Mode == kHeatModeCubic, parts = Mode == kHeatModeParts;
    const bool bilinear = !cubic && !parts && H.count == 1;   // renderPartAffinities' one PAF
    // the channels drawn, from H.channel, in items of one channel or a PAF's two
    const int unit = cubic || parts ? 1 : 2;
    const int total = cubic ? 1 : H.count * unit;
    // what a pass stages: the kind's taps around the tile's bases, as many items as fit
    HeatWindow W = heat_window(H, win, cubic ? 1 : 0, cubic ? 2 : (parts || bilinear ? 1 : 0), unit);
    int chunk = total;
    if (W.w > 0) {
        chunk = min(total, kRenderHeatWindow / (W.w * W.h));
        chunk -= chunk % unit;
    }
    // the kind's sampler once more, in scalars, for the loop over missed taps
    const HeatSampler S{cubic ? 16 : (parts ? 1 : (bilinear ? 8 : 2)), cubic ? 4 : (bilinear ? 2 : 0),
                        cubic ? 3 : (bilinear ? 1 : 0), cubic ? 2 : (bilinear ? 1 : 0),
                        cubic ? 3 : (bilinear ? 1 : 0)};
    // the pixel's base: cubicSequentialData's, or the all-parts render's flat index p * area + off
    // back to (plane p + dq, y, x)
    const HeatBase hb = heat_base(xs, ys, hw, hh);
    int bx = cubic ? hb.x1 - 1 : hb.x1, by = cubic ? hb.y1 - 1 : hb.y1, dq = 0;
    if (parts) {
        const int off = (int)heat_maps_offset(xs, ys, hw, hh);   // <= area + hw (the launcher's bound)
        const int area = hw * hh;
        dq = off / area;
        const int rem = off - dq * area;
        by = rem / hw;
        bx = rem - by * hw;
    }
    float c[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int c0 = 0; c0 < total; c0 += chunk) {
        const int staged = min(chunk, total - c0);
        heat_stage(H, W, win, f, H.channel + c0, staged);
        if (!t.inside) continue;
        int color = parts ? c0 % H.ncolors : 0;   // the part's color row, i % ncolors
        int i = c0;
        if (parts) {
            // the parts whose plane i + dq is staged at the pixel's (bx, by) -- all of the pass for
            // nearly every pixel -- straight from the window: independent LDS reads
            const unsigned wx = (unsigned)(bx - W.x0), wy = (unsigned)(by - W.y0);
            const int fast = wx < (unsigned)W.w && wy < (unsigned)W.h
                                 ? min(c0 + staged, H.count) - dq   // planes c0 .. c0 + staged - 1
                                 : c0;
            const float* at = W.win + wy * W.w + wx + dq * W.w * W.h;
#pragma unroll 4
            for (; i < fast; ++i) {
                heat_maps_add(c, at[(i - c0) * W.w * W.h], H.colors + color * 3);
                color = color + 1 == H.ncolors ? 0 : color + 1;
            }
        }
#pragma unroll 1
        for (; i < c0 + staged; i += unit) {
            int ch = H.channel + i, x = bx, y = by;
            if (parts && i + dq > H.count - 1) {   // past the end of the parts: the stack's last value
                ch = H.count - 1;
                x = hw - 1;
                y = hh - 1;
            } else if (parts) {
                ch = i + dq;
            }
            float v[kHeatMaxTaps];
            unsigned miss;
            if (cubic) miss = heat_gather_window(v, kSampleBicubic, W, ch, x, y, hw, hh);
            else if (parts) miss = heat_gather_window(v, kSampleOne, W, ch, x, y, hw, hh);
            else if (bilinear) miss = heat_gather_window(v, kSamplePaf, W, ch, x, y, hw, hh);
            else miss = heat_gather_window(v, kSamplePafBase, W, ch, x, y, hw, hh);
            heat_gather_missed(v, miss, S, H, f, ch, x, y);
            if (cubic) {
                const float h = heat_bicubic(v, hb.dx, hb.dy);
                color_heat(c, H.kind == kHeatDistance ? fabsf(h) : h);
            } else if (parts) {
                heat_maps_add(c, v[0], H.colors + color * 3);
                color = color + 1 == H.ncolors ? 0 : color + 1;
            } else {
                paf_add(c, v, v + (bilinear ? 4 : 1), hb.dx, hb.dy, bilinear);
            }
        }
    }
    float px[3] = {b, g, r};
    blend_bgr(px, c, H.alpha);
    b = px[0];
    g = px[1];
    r = px[2];
}

// Heat: the heat layer's mode (kHeatModeNone: the keypoint-only kernel carries none of it);
// YuvOut: an NV12 / I420 destination -- a template parameter, not a branch on a.out.format: with the
// branch the BGR destination measured 0.9 % slower than before it existed; which of
// the two YUV layouts is a run-time, grid-uniform choice (a.out.cpix)
template <int K, int Heat, bool Yuv, bool YuvOut>
__global__ __launch_bounds__(256) void render_frames_kernel(const RenderFramesArgs a)
{
    __shared__ unsigned short plist[kRenderMaxPeople];
    __shared__ float4 items[256][4];
    __shared__ int wcount[4];
    const int f = blockIdx.z;
    const RenderTile t = render_tile(a.w, a.h);
    // 1. the pixel of the output image, in registers from here to the store
    float b = 0.f, g = 0.f, r = 0.f;
    if (t.inside && a.blend) {
        int u[3];
        output_pixel<K, Yuv>(u, a.warp, f, t.x, t.y);
        b = (float)u[0];
        g = (float)u[1];
        r = (float)u[2];
    }
    // 2. the heat layer; `items` is its window
    if constexpr (Heat != kHeatModeNone) {
        render_heat_pixel<Heat>(a.heat, t, f, reinterpret_cast<float*>(items), b, g, r);
        __syncthreads();   // the keypoint layers rewrite items
    }
    // 3. every layer in order on the frame's own people
    for (int l = 0; l < a.nlayers; ++l) {
        const RenderFramesLayer& L = a.layer[l];
        const int first = L.offsets[f], people = L.offsets[f + 1] - first;
        render_view_pixel(render_view(L.geom, L.total, first, people, L.npairs, L.parts, L.colors,
                                      L.alpha),
                          t, plist, items, wcount, b, g, r);
    }
    // 4. OpOutputToCvMat's cast
    const unsigned cb = cast_u8(b, a.cast), cg = cast_u8(g, a.cast), cr = cast_u8(r, a.cast);
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int rows = min(kTileH, a.h - ty0), cols = min(kTileW, a.w - tx0);
    // 5. an NV12 / I420 destination: the cast bytes become samples and leave (yuv_out_dev.h);
    //    `items` is idle -- every use of it ended at a barrier -- and stages the tile
    if constexpr (YuvOut) {
        yuv_store_tile(a, f, t.x, t.y, t.inside, cb, cg, cr, reinterpret_cast<uint8_t*>(items),
                       threadIdx.x, tx0, ty0, rows, cols);
        return;
    }
    // 6. a BGR destination.  (Written out here, not a helper like step 5: as a function of its own
    //    these lines are optimised before they are inlined -- the lane's / 24 and % 24 come out 16
    //    bits wide -- and all 24 BGR kernels become other code, which nothing here has measured.)
    if (!a.dst_aligned) {
        if (t.inside) {
            uint8_t* d = a.dst + (size_t)f * a.dst_frame + (size_t)t.y * a.dst_step + (size_t)t.x * 3;
            d[0] = (uint8_t)cb;
            d[1] = (uint8_t)cg;
            d[2] = (uint8_t)cr;
        }
        return;
    }
    // rows on 4-byte boundaries (a tile starts at byte 96 * blockIdx.x of its rows): the tile's
    // 8 x 96 bytes go through LDS -- `items` is idle, every use of it ended at a barrier -- and
    // leave as 4-byte stores, 24 lanes a row; a row's last 1..3 bytes, if any, as bytes
    uint8_t* stage = reinterpret_cast<uint8_t*>(items);
    uint8_t* mine = stage + threadIdx.x * 3;   // (threadIdx.x / 32) * 96 + (threadIdx.x % 32) * 3
    mine[0] = (uint8_t)cb;
    mine[1] = (uint8_t)cg;
    mine[2] = (uint8_t)cr;
    __syncthreads();
    const int row_bytes = cols * 3;
    const int row = threadIdx.x / 24, o = (threadIdx.x % 24) * 4;
    if (row < rows && o < row_bytes) {   // row < 8 only for threadIdx.x < 192
        uint8_t* d = a.dst + (size_t)f * a.dst_frame + (size_t)(ty0 + row) * a.dst_step +
                     (size_t)tx0 * 3 + o;
        const uint8_t* s = stage + row * (kTileW * 3) + o;
        if (o + 4 <= row_bytes) {
            *reinterpret_cast<unsigned*>(d) = *reinterpret_cast<const unsigned*>(s);
        } else {
            for (int i = 0; i < row_bytes - o; ++i) d[i] = s[i];
        }
    }
}

dim3 tiles(int w, int h)
{
    return dim3((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH));
}

}  // namespace

size_t render_geom_floats(int people, int parts, int npairs)
{
    return (size_t)people * (8 + (size_t)npairs * 8 + (size_t)parts * 8);
}

void launch_render_prep(const RenderKeypointsArgs& a, hipStream_t stream)
{
    if (a.people <= 0) return;
    render_prep_kernel<<<a.people, 64, 0, stream>>>(a);
    OPK_LAUNCH_CHECK();
}

void launch_render_keypoints(const RenderKeypointsArgs& a, hipStream_t stream)
{
    if (a.w <= 0 || a.h <= 0) return;
    launch_render_prep(a, stream);
    render_keypoints_kernel<<<tiles(a.w, a.h), kTileW * kTileH, 0, stream>>>(a);
    OPK_LAUNCH_CHECK();
}

namespace {

// the (tiles_x, tiles_y, n) grid of the batch kernels
dim3 batch_tiles(int w, int h, int n)
{
    dim3 g = tiles(w, h);
    OPK_CHECK_ARG(g.y <= 65535u && n <= 65535, "more than 65535 tile rows or frames");
    g.z = (unsigned)n;
    return g;
}

void check_warp(const FrameWarp& wp, int w, int h)
{
    const FrameSource& fs = wp.src;
    OPK_CHECK_ARG(fs.plane[0] && fs.w > 0 && fs.h > 0, "empty frame");
    check_frames(fs);
    OPK_CHECK_ARG(wp.ksize == 0 || wp.ksize == 2 || wp.ksize == 4, "copy, linear or cubic");
    OPK_CHECK_ARG(wp.ksize != 0 || (w == fs.w && h == fs.h), "a copy keeps the size");
    OPK_CHECK_ARG(wp.ksize == 0 || (wp.xtab && wp.ytab && wp.wtab), "NULL warp table");
}

}  // namespace

void launch_cvmat_to_output(float* dst, int n, int w, int h, const FrameWarp& wp,
                            hipStream_t stream)
{
    OPK_CHECK_ARG(dst && n > 0 && w > 0 && h > 0, "empty output image");
    check_warp(wp, w, h);
    const dim3 grid = batch_tiles(w, h, n), block(kTileW * kTileH);
#define OPK_LAUNCH_OUTPUT(K)                                                                     \
    do {                                                                                         \
        if (wp.src.format == kFramesBgr)                                                         \
            hipLaunchKernelGGL((cvmat_to_output_kernel<K, false>), grid, block, 0, stream, dst, w, \
                               h, wp);                                                           \
        else                                                                                     \
            hipLaunchKernelGGL((cvmat_to_output_kernel<K, true>), grid, block, 0, stream, dst, w,  \
                               h, wp);                                                           \
    } while (0)
    if (wp.ksize == 0)
        OPK_LAUNCH_OUTPUT(0);
    else if (wp.ksize == 2)
        OPK_LAUNCH_OUTPUT(2);
    else
        OPK_LAUNCH_OUTPUT(4);
#undef OPK_LAUNCH_OUTPUT
    OPK_LAUNCH_CHECK();
}

void launch_output_to_cvmat(uint8_t* dst, size_t dst_step, const float* src, int n, int w, int h,
                            int cast, hipStream_t stream)
{
    OPK_CHECK_ARG(dst && src && n > 0 && w > 0 && h > 0, "empty output image");
    OPK_CHECK_ARG(w <= (1 << 29) / 3, "row too long");
    OPK_CHECK_ARG(dst_step >= (size_t)w * 3, "row step shorter than the row");
    OPK_CHECK_ARG(cast == 0 || cast == 1, "unknown cast");
    OPK_CHECK_ARG(h <= 65535 && n <= 65535, "more than 65535 rows or frames");
    const int row = w * 3;
    // four values per thread: a row of floats starts 16-byte aligned when w*3 is a multiple of
    // 4, a row of bytes 4-byte aligned when dst_step is; the last store ends at w*3 exactly
    const bool vec = row % 4 == 0 && dst_step % 4 == 0 && (uintptr_t)dst % 4 == 0 &&
                     (uintptr_t)src % 16 == 0;
    const int per_block = 256 * (vec ? 4 : 1);
    const dim3 grid((unsigned)((row + per_block - 1) / per_block), (unsigned)h, (unsigned)n);
    if (vec)
        hipLaunchKernelGGL(output_to_cvmat_kernel<true>, grid, dim3(256), 0, stream, dst, dst_step,
                           src, row, h, cast);
    else
        hipLaunchKernelGGL(output_to_cvmat_kernel<false>, grid, dim3(256), 0, stream, dst,
                           dst_step, src, row, h, cast);
    OPK_LAUNCH_CHECK();
}

void launch_render_frames(const RenderFramesArgs& args, hipStream_t stream)
{
    RenderFramesArgs a = args;
    FrameDest& D = a.out;
    OPK_CHECK_ARG(D.plane[0] && a.n > 0 && a.w > 0 && a.h > 0, "empty output image");
    OPK_CHECK_ARG(D.n == a.n && D.w == a.w && D.h == a.h, "destination frame count or size");
    check_frames(D);
    const bool yuv_out = D.format != kFramesBgr;
    a.dst_aligned = frames_aligned(D, 4);
    a.dst = D.plane[0];
    a.dst_step = D.step;
    a.dst_frame = D.frame[0];
    // the store route in the launch log: a4 = the 4-byte stores from the stage
    if (!yuv_out)
        note_launch(a.dst_aligned ? "render_frames<a4>" : "render_frames");
    else if (D.format == kFramesNv12)
        note_launch(a.dst_aligned ? "render_frames<a4,nv12>" : "render_frames<nv12>");
    else
        note_launch(a.dst_aligned ? "render_frames<a4,i420>" : "render_frames<i420>");
    OPK_CHECK_ARG(a.cast == 0 || a.cast == 1, "unknown cast");
    OPK_CHECK_ARG(a.nlayers >= 0 && a.nlayers <= kRenderMaxLayers, "too many layers");
    for (int l = 0; l < a.nlayers; ++l)
        OPK_CHECK_ARG(a.layer[l].offsets && (a.layer[l].total == 0 || a.layer[l].geom),
                      "NULL layer");
    check_warp(a.warp, a.w, a.h);
    RenderFramesHeat& H = a.heat;
    const bool heat = H.kind != kHeatNone;
    if (heat) {
        OPK_CHECK_ARG(H.kind >= kHeatPart && H.kind <= kHeatDistance, "unknown heat kind");
        OPK_CHECK_ARG(a.blend, "the heat layer blends with the frame");
        const HeatMap& M = H.map;
        OPK_CHECK_ARG(M.w > 0 && M.h > 0 && M.channels > 0, "empty heat map");
        OPK_CHECK_ARG(M.heat || (M.nsrc >= 1 && M.nsrc <= kMaxResizeSources), "heat map sources");
        // plane indices and a plane's offsets (the all-parts render's reaches area + w) are ints
        OPK_CHECK_ARG((size_t)M.w * M.h <= (1u << 30) &&
                          (size_t)a.n * M.channels <= (size_t)INT32_MAX,
                      "heat stack too large");
        const bool pair = H.kind == kHeatPaf || H.kind == kHeatPafs;
        const int first = H.kind == kHeatParts ? 0 : H.channel;
        const int used = H.kind == kHeatParts ? H.count : (pair ? 2 * H.count : 1);
        OPK_CHECK_ARG(H.count >= 1 || !(pair || H.kind == kHeatParts), "no channel to draw");
        OPK_CHECK_ARG(first >= 0 && used <= M.channels - first, "channel outside the heat stack");
        OPK_CHECK_ARG(H.kind != kHeatParts || (H.colors && H.ncolors > 0), "NULL colors");
        // RENDER_HEAT_STAGE=0 (dev A/B): every pixel evaluates its own samples
        H.staged = dev_switch("RENDER_HEAT_STAGE", 1) != 0 &&
                   render_heat_staged(H.kind == kHeatPafs && H.count == 1 ? kHeatPaf : H.kind, H.scale);
    }
    const dim3 grid = batch_tiles(a.w, a.h, a.n), block(kTileW * kTileH);
#define OPK_LAUNCH_FRAMES_OUT(K, M, Y)                                                             \
    do {                                                                                           \
        if (!yuv_out)                                                                              \
            hipLaunchKernelGGL((render_frames_kernel<K, M, Y, false>), grid, block, 0, stream, a); \
        else                                                                                       \
            hipLaunchKernelGGL((render_frames_kernel<K, M, Y, true>), grid, block, 0, stream, a);  \
    } while (0)
#define OPK_LAUNCH_FRAMES_MODE(K, M)               \
    do {                                           \
        if (a.warp.src.format == kFramesBgr)       \
            OPK_LAUNCH_FRAMES_OUT(K, M, false);    \
        else                                       \
            OPK_LAUNCH_FRAMES_OUT(K, M, true);     \
    } while (0)
#define OPK_LAUNCH_FRAMES(K)                                                                       \
    do {                                                                                           \
        if (!heat)                                                                                 \
            OPK_LAUNCH_FRAMES_MODE(K, kHeatModeNone);                                              \
        else if (H.kind == kHeatPart || H.kind == kHeatDistance)                                   \
            OPK_LAUNCH_FRAMES_MODE(K, kHeatModeCubic);                                             \
        else if (H.kind == kHeatParts)                                                             \
            OPK_LAUNCH_FRAMES_MODE(K, kHeatModeParts);                                             \
        else                                                                                       \
            OPK_LAUNCH_FRAMES_MODE(K, kHeatModePaf);                                               \
    } while (0)
    if (a.warp.ksize == 0)
        OPK_LAUNCH_FRAMES(0);
    else if (a.warp.ksize == 2)
        OPK_LAUNCH_FRAMES(2);
    else
        OPK_LAUNCH_FRAMES(4);
#undef OPK_LAUNCH_FRAMES_OUT
#undef OPK_LAUNCH_FRAMES_MODE
#undef OPK_LAUNCH_FRAMES
    OPK_LAUNCH_CHECK();
}

bool render_heat_staged(int kind, float scale)
{
    // heat_window's rectangle: the bases of a tile's first and last pixel are at most
    // floor(31 / scale) + 1 (8 rows: floor(7 / scale) + 1) apart -- one more allows for the
    // rounding of the two source coordinates --, plus the kind's taps
    int taps = 0, planes = 1;
    if (kind == kHeatPart || kind == kHeatDistance) taps = 3;
    else if (kind == kHeatParts) taps = 1;
    else if (kind == kHeatPaf) taps = 1, planes = 2;
    else if (kind == kHeatPafs) planes = 2;
    else return false;
    if (!(scale > 0.f) || !std::isfinite(scale)) return false;
    const double w = std::floor((kTileW - 1) / (double)scale) + 3 + taps;
    const double h = std::floor((kTileH - 1) / (double)scale) + 3 + taps;
    return w * h * planes <= kRenderHeatWindow;
}

void launch_render_heat_map(const RenderHeatArgs& a, int part, bool abs_value, hipStream_t stream)
{
    if (a.w <= 0 || a.h <= 0) return;
    render_heat_map_kernel<<<tiles(a.w, a.h), kTileW * kTileH, 0, stream>>>(a, part, abs_value);
    OPK_LAUNCH_CHECK();
}

void launch_render_heat_maps(const RenderHeatArgs& a, int parts, const float* colors, int ncolors,
                             hipStream_t stream)
{
    if (a.w <= 0 || a.h <= 0) return;
    render_heat_maps_kernel<<<tiles(a.w, a.h), kTileW * kTileH, 0, stream>>>(a, parts, colors,
                                                                              ncolors);
    OPK_LAUNCH_CHECK();
}

void launch_render_pafs(const RenderHeatArgs& a, int first, int count, hipStream_t stream)
{
    if (a.w <= 0 || a.h <= 0) return;
    render_pafs_kernel<<<tiles(a.w, a.h), kTileW * kTileH, 0, stream>>>(a, first, count);
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
