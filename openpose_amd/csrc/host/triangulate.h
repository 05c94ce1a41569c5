// triangulate.h -- 3-D keypoints from a camera rig (include/opk.h): the checked rig, the host
// route and the device route of one reconstructArray.
#pragma once
#include <hip/hip_runtime.h>

#include "../kernels/triangulate_dev.h"

struct opk_rig;   // include/opk.h

namespace opk {

struct Context;

// the rig checked as include/opk.h states (an OPK_ERR_ARG error otherwise), min_views resolved
TriRig make_rig(const ::opk_rig* rig);
// out[3][4] = K[3][3] * Rt[3][4], sequential sums
void camera_matrix(const double* K, const double* Rt, double* out);
// opk_triangulate_host; errors / dropped may be NULL
void triangulate_host(const TriRig& rig, int steps, int parts, const float* kp, const int* present,
                      float* xyz, int* status, double* errors, int* dropped);
// opk_triangulate: device buffers, enqueued on ctx's stream (kernels/triangulate.hip)
void triangulate(Context* ctx, const TriRig& rig, int steps, int parts, const float* kp,
                 const int* present, float* xyz, int* status, double* errors, int* dropped);
// kernels/triangulate.hip: the point launch and the acceptance launch; err is required
void launch_triangulate(const TriRig& rig, int steps, int parts, const float* kp, const int* present,
                        float* xyz, int* status, double* err, int* dropped, hipStream_t stream);

}  // namespace opk
