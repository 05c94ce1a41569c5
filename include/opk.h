/*
 * opk.h -- C-ABI of libopk_hip.so, the MI355X (gfx950) implementation of OpenPose's per-frame
 * body hot path: BODY_25 CNN forward -> resizeAndMerge -> NMS -> bodyPartConnector.
 *
 * Plain C: pointers, sizes and int status codes, no C++ or torch types.  Every function returns
 * OPK_OK (0) or an error code; opk_last_error() returns the calling thread's message (the C++ shim
 * in include/openpose_amd/ converts it into op::error(), the reference's error convention,
 * errorAndLog.cpp:158-233).  "dev" pointers are device (HBM) pointers; "host" pointers host memory.
 * All device work is enqueued on the context's hipStream_t; functions that hand results to the host
 * synchronise that stream (the points where the reference reads cpu_data()).
 *
 * Each entry point names the reference interface it replaces (paths under /root/reference/).
 */
#ifndef OPK_H
#define OPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPK_OK 0
#define OPK_ERR_ARG 1      /* invalid argument (reference: op::error(...) sanity checks)       */
#define OPK_ERR_HIP 2      /* HIP runtime error (reference: cudaCheck, gpu/cuda.cpp:18-26)      */
#define OPK_ERR_STATE 3    /* call out of order (e.g. forward before weights)                   */
#define OPK_ERR_UNSUPPORTED 4

/* PoseModel values (include/openpose/pose/enumClasses.hpp:9-30); the tables of every model are
 * generated from the reference's poseParameters.cpp (tools/gen_pose_tables.py) */
#define OPK_BODY_25 0
#define OPK_COCO_18 1
#define OPK_MPI_15 2
#define OPK_MPI_15_4 3
#define OPK_BODY_19 4
#define OPK_BODY_19_X2 5
#define OPK_BODY_19N 6
#define OPK_BODY_25E 7
#define OPK_CAR_12 8
#define OPK_BODY_25D 9
#define OPK_BODY_23 10
#define OPK_CAR_22 11
#define OPK_BODY_19E 12
#define OPK_BODY_25B 13
#define OPK_BODY_135 14

/* Connector semantics.  OPK_CONNECT_CPU: connectBodyPartsCpu (bodyPartConnectorBase.cpp:1327-1377,
 * per-pair greedy matching; the reference accepts BODY_25 / COCO_18 / MPI_15(_4) only).
 * OPK_CONNECT_GPU: connectBodyPartsGpu's host assembly (bodyPartConnectorBase.cu:147-250:
 * pafPtrIntoVector's global sort + pafVectorIntoPeopleVector; every model, BODY_135 included).
 * Pair scores are the same getScoreAB integrals in both. */
#define OPK_CONNECT_CPU 0
#define OPK_CONNECT_GPU 1

const char* opk_last_error(void);
int opk_version(void);

/* ---- context: one per GPU worker thread (reference: one PoseExtractorCaffe per GPU thread,
 *      wrapperAuxiliary.hpp:328-337; device bound at init like Caffe::SetDevice, netCaffe.cpp:169) */
typedef struct opk_ctx opk_ctx;
/* device -1: host-only context (graph planning, opk_net_conv_info; no device work) */
int opk_ctx_create(int device, void* hip_stream /* used as given; NULL = the null stream */,
                   opk_ctx** out);
/* same, with a private non-blocking stream owned (and destroyed) by the context */
int opk_ctx_create_private_stream(int device, opk_ctx** out);
int opk_ctx_destroy(opk_ctx* ctx);
int opk_ctx_stream(opk_ctx* ctx, void** hip_stream);
/* waits for the context stream and for the side streams of the context's objects (a pose
 * pipeline's post-processing stream) */
int opk_sync(opk_ctx* ctx);
int opk_malloc(opk_ctx* ctx, void** dev, size_t bytes);
int opk_free(opk_ctx* ctx, void* dev);
int opk_memset(opk_ctx* ctx, void* dev, int value, size_t bytes);
int opk_memcpy_h2d(opk_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int opk_memcpy_d2h(opk_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes); /* syncs */
/* element type conversion on the device, on the context stream: OPK_F32 <-> OPK_F64 (double -> float
 * rounds to nearest).  The plugin functions' double instantiations (resizeAndMergeBase.cu:575-581,
 * nmsBase.cu:353-358, bodyPartConnectorBase.cu:252-266, which compute in double) run the float
 * kernels between two conversions here (integration/openpose_hip_shim.cpp): the results are the
 * float instantiation's, widened. */
#define OPK_F32 0
#define OPK_F64 1
#define OPK_U8 2   /* a destination type of opk_pose_heatmaps_copy_range only */
int opk_convert(opk_ctx* ctx, void* dst_dev, int dst_type, const void* src_dev, int src_type,
                size_t count);

/* ---- resizeAndMerge: replaces op::resizeAndMergeGpu<float>
 *      (include/openpose/net/resizeAndMergeBase.hpp:17-20) with resizeAndMergeCpu numerics
 *      (src/openpose/net/resizeAndMergeBase.cpp:9-113: cv::resize INTER_CUBIC per plane, then the
 *      multi-scale average).  target_size / source_sizes are NCHW {N, C, H, W}; N frames are
 *      processed as a batch (the reference merges N into one frame only for N == 1 per scale).
 *      scale_ratios is accepted for signature parity and ignored, as in the CPU path (:18). */
int opk_resize_and_merge(opk_ctx* ctx, float* target_dev, const float* const* sources_dev,
                         int num_sources, const int target_size[4], const int* source_sizes,
                         const float* scale_ratios);

/* ---- NMS: replaces op::nmsGpu<float> (include/openpose/net/nmsBase.hpp:14-16) with nmsCpu
 *      numerics (src/openpose/net/nmsBase.cpp:7-170).  target_size = {N, parts, maxPeaks+1, 3},
 *      source_size = {N, C, H, W}; only the first `parts` planes of each frame are scanned.
 *      kernel_scratch (the reference's int peak map) may be NULL: this implementation never
 *      materialises it (peaks are appended to small per-plane candidate lists owned by the
 *      context, then sorted into raster order per plane). */
int opk_nms(opk_ctx* ctx, float* target_dev, int* kernel_scratch_dev, const float* source_dev,
            float threshold, const int target_size[4], const int source_size[4],
            float offset_x, float offset_y);

/* ---- Heat-map semantics of the reference's two builds (resize + NMS).
 * OPK_MAPS_CPU (the default everywhere): resizeAndMergeCpu + nmsCpu, as above.
 * OPK_MAPS_CUDA: what a CUDA build of the reference computes --
 *   resizeAndMergeGpu (src/openpose/net/resizeAndMergeBase.cu:105-162,274-495): Catmull-Rom
 *   bicubic (cubicInterpolate/bicubicInterpolate, include/openpose_private/gpu/cuda.hu:92-145) with
 *   the clamped base, one source only at x8 (or identity; other ratios are the reference's
 *   "Kernel only implemented for 8x resize" error), several sources scaled by
 *   (W/W0) / (scale_ratios[i] / scale_ratios[0]) and averaged as sum / N (scale_ratios required);
 *   nmsGpu (src/openpose/net/nmsBase.cu:50-90,161-240): interior pixels only, strictly greater
 *   than all 8 neighbours, centroid sums fused multiply-adds (nvcc's default contraction).
 * The expressions are evaluated as written, each operation rounded (nvcc's exact contraction of the
 * cubic polynomial is not reproducible without the CUDA toolchain: parity unpinned). */
#define OPK_MAPS_CPU 0
#define OPK_MAPS_CUDA 1
int opk_resize_and_merge_semantics(opk_ctx* ctx, float* target_dev, const float* const* sources_dev,
                                   int num_sources, const int target_size[4],
                                   const int* source_sizes, const float* scale_ratios,
                                   int semantics);
int opk_nms_semantics(opk_ctx* ctx, float* target_dev, int* kernel_scratch_dev,
                      const float* source_dev, float threshold, const int target_size[4],
                      const int source_size[4], float offset_x, float offset_y, int semantics);

/* ---- PAF pair scores: the pafScoreKernel stage of op::connectBodyPartsGpu
 *      (src/openpose/net/bodyPartConnectorBase.cu:107-145) computed with the CPU path's getScoreAB
 *      numerics (bodyPartConnectorBase.cpp:12-75: clamp to the map, 0 on rejection).
 *      pair_scores_dev: [N][numPairs][maxPeaks][maxPeaks]; only i < nA, j < nB are written.
 *      heat: [N][heat_channels][heat_h][heat_w]; peaks: [N][parts][maxPeaks+1][3]. */
int opk_paf_scores(opk_ctx* ctx, float* pair_scores_dev, const float* heat_dev,
                   const float* peaks_dev, int num_frames, int pose_model, int heat_channels,
                   int heat_h, int heat_w, int max_peaks, float inter_threshold,
                   float inter_min_above_threshold, float default_nms_threshold);

/* The same scores on the lazy heat map the pipeline scores (opk_pose_*: the merged map is never
 * written; every sample is resized from the net outputs), built from `num_sources` net outputs
 * (source_sizes: {N, C, h, w} each) at target_h x target_w with heat-map `semantics`
 * (scale_ratios: as opk_resize_and_merge_semantics).  rec_floats 0: out_dev is the dense
 * [N][numPairs][maxPeaks][maxPeaks] array of opk_paf_scores.  rec_floats > 1: out_dev holds one
 * record of rec_floats floats per frame, as the pipeline's: [0] = the number of scores (-1 when
 * they do not fit, nothing else written), then the nA x nB scores of pair 0, pair 1, ...
 * *staged_bytes (may be NULL): the bytes of a workgroup's on-chip copy of the sources, 0 when the
 * kernels read them from memory. */
int opk_paf_scores_sources(opk_ctx* ctx, float* out_dev, int rec_floats,
                           const float* const* sources_dev, int num_sources,
                           const int* source_sizes, int target_h, int target_w, int semantics,
                           const float* scale_ratios, const float* peaks_dev, int pose_model,
                           int max_peaks, float inter_threshold, float inter_min_above_threshold,
                           float default_nms_threshold, size_t* staged_bytes);

/* ---- connectBodyParts: replaces op::connectBodyPartsGpu<float>
 *      (include/openpose/net/bodyPartConnectorBase.hpp:17-24) with connectBodyPartsCpu semantics
 *      (bodyPartConnectorBase.cpp:1327-1377): GPU pair scores + host people assembly.
 *      keypoints_host [max_people][parts][3], scores_host [max_people]; *num_people gets the true
 *      count (rows beyond max_people are dropped). */
int opk_connect_body_parts(opk_ctx* ctx, float* keypoints_host, float* scores_host,
                           int max_people, int* num_people, const float* heat_dev,
                           const float* peaks_dev, int pose_model, int heat_channels, int heat_h,
                           int heat_w, int max_peaks, float inter_min_above_threshold,
                           float inter_threshold, int min_subset_cnt, float min_subset_score,
                           float default_nms_threshold, float scale_factor,
                           int maximize_positives);

/* Host-only people assembly from host peaks + host dense pair scores
 * (createPeopleVector's precomputed-score input, bodyPartConnectorBase.cpp:321-340, then
 * removePeopleBelowThresholdsAndFillFaces + peopleVectorToPeopleArray :720-934). */
int opk_assemble_people(float* keypoints_host, float* scores_host, int max_people,
                        int* num_people, const float* pair_scores_host,
                        const float* peaks_host, int pose_model, int max_peaks,
                        int min_subset_cnt, float min_subset_score, float scale_factor,
                        int maximize_positives);

/* The same two with a connector semantics (OPK_CONNECT_CPU / OPK_CONNECT_GPU); the GPU
 * semantics replace op::connectBodyPartsGpu<float> for every model. */
int opk_assemble_people_semantics(float* keypoints_host, float* scores_host, int max_people,
                                  int* num_people, const float* pair_scores_host,
                                  const float* peaks_host, int pose_model, int max_peaks,
                                  int min_subset_cnt, float min_subset_score, float scale_factor,
                                  int maximize_positives, int semantics);
int opk_connect_body_parts_semantics(opk_ctx* ctx, float* keypoints_host, float* scores_host,
                                     int max_people, int* num_people, const float* heat_dev,
                                     const float* peaks_dev, int pose_model, int heat_channels,
                                     int heat_h, int heat_w, int max_peaks,
                                     float inter_min_above_threshold, float inter_threshold,
                                     int min_subset_cnt, float min_subset_score,
                                     float default_nms_threshold, float scale_factor,
                                     int maximize_positives, int semantics);

/* ---- Keypoint post-steps (host arrays [people][parts][3]).
 * opk_scale_keypoints replaces op::KeypointScaler::scale (src/openpose/core/keypointScaler.cpp:64-95;
 * getScaleAndOffset :6-45): scale_mode = op::ScaleMode (0 InputResolution = unchanged,
 * 1 NetOutputResolution, 2 OutputResolution, 3/4 ZeroToOne(FixedAspect), 5/6 PlusMinusOne(...)).
 * opk_keep_top_n_people replaces op::KeepTopNPeople::keepTopPeople (keepTopNPeople.cpp:16-86,
 * --number_people_max): people ranked by score * sqrt(keypoint box area) and the top max_people
 * kept in their original order; *out_people = rows written (people itself when no cut is needed),
 * out_index_host (may be NULL) = source person of each row. */
int opk_scale_keypoints(float* keypoints_host, int people, int parts, int scale_mode,
                        double scale_input_to_output, double scale_net_to_output, int producer_w,
                        int producer_h);
int opk_keep_top_n_people(const float* keypoints_host, int people, int parts,
                          const float* scores_host, int max_people, float* out_keypoints_host,
                          int* out_index_host, int* out_people);

/* ---- People JSON (--write_json).  One keypoint array of the reference's keypointVector
 * (WPeopleJsonSaver::workConsumer, include/openpose/filestream/wPeopleJsonSaver.hpp:75-88):
 * name ("person_id", "pose_keypoints_2d", ...), ndims 0 (empty op::Array), 1 ([people], e.g. the
 * person ids as float) or 3 ([people][parts][dims]); host data. */
typedef struct opk_json_keypoints {
    const char* name;
    const float* data;
    int ndims, people, parts, dims;
} opk_json_keypoints;
/* opk_people_json replaces op::savePeopleJson(keypointVector, candidates, fileName, humanReadable)
 * (src/openpose/filestream/fileStream.cpp:306-344, JsonOfstream formatting): writes the file's text
 * (no terminating NUL counted) into out_host when *len + 1 <= capacity (out_host may be NULL to
 * query), *len = its length.  candidates_host: n_parts lists of [x, y, score] back to back,
 * candidate_counts_host[part] each (the Datum's poseCandidates; n_parts 0 = none, no
 * "part_candidates" key).  opk_save_people_json writes the same text to path (PeopleJsonSaver::save,
 * peopleJsonSaver.cpp:15-30, with the ".json" already in path). */
int opk_people_json(const opk_json_keypoints* arrays, int n_arrays, const float* candidates_host,
                    const int* candidate_counts_host, int n_parts, int human_readable,
                    char* out_host, size_t capacity, size_t* len);
int opk_save_people_json(const char* path, const opk_json_keypoints* arrays, int n_arrays,
                         const float* candidates_host, const int* candidate_counts_host,
                         int n_parts, int human_readable);

/* Pose tables (getPoseNumberBodyParts, addBkgChannel, getPosePartPairs, getPoseMapIndex;
 * poseParameters.hpp:17-34).  Any output pointer may be NULL; pairs gets 2*npairs entries,
 * map_idx the model's map-index entries (heat_channels - parts - bkg). */
int opk_pose_model_info(int pose_model, int* parts, int* bkg, int* npairs, int* heat_channels,
                        int* pairs, int* map_idx);
/* getPoseDefaultNmsThreshold / getPoseDefaultConnectInterThreshold (poseParameters.hpp:29-31) */
int opk_pose_default_thresholds(int pose_model, int maximize_positives, float* nms_threshold,
                                float* inter_threshold);

/* ---- Frame -> net input.
 * opk_scale_and_size replaces op::ScaleAndSizeExtractor::extract
 *      (include/openpose/core/scaleAndSizeExtractor.hpp:17-18, scaleAndSizeExtractor.cpp:37-105):
 *      net_w or net_h <= 0 derives that side from the frame's aspect ratio (-1x368), bounded at
 *      16:9 times dynamic_behavior when it is > 0 (--net_resolution_dynamic); scales[i] =
 *      scaleInputToNetInputs, net_sizes[2i], [2i+1] = netInputSizes (w, h), i < scale_number.
 * opk_cvmat_to_input replaces op::CvMatToOpInput::createArray for one scale
 *      (include/openpose/core/cvMatToOpInput.hpp:17-19, cvMatToOpInput.cpp:63-98), for a batch:
 *      frames_dev = n BGR uint8 frames [height][step bytes] (step 0 = width*3), input_dev =
 *      [n][3][net_h][net_w] fp32: cv::warpAffine(diag(scale)) with OpenCV's fixed-point 8-bit
 *      arithmetic (INTER_LINEAR for scale <= 1, INTER_CUBIC above; zero border), then
 *      u/256 - 0.5 when normalize == 1 (uCharCvMatToFloatPtr, openCv.cpp:57-150). */
int opk_scale_and_size(int in_w, int in_h, int net_w, int net_h, float dynamic_behavior,
                       int scale_number, double scale_gap, double* scales, int* net_sizes);
int opk_cvmat_to_input(opk_ctx* ctx, float* input_dev, const uint8_t* frames_dev, int n, int width,
                       int height, size_t step, double scale, int net_w, int net_h, int normalize);

/* ---- Frames as the decoders leave them: packed BGR, or YUV 4:2:0 as NV12 (the hardware decode
 * engines' surfaces) or I420 (software decoders).  Every function that takes `frames_dev, n, width,
 * height, step` has a `_fmt` form taking this descriptor instead; the pointer-taking forms are the
 * `_fmt` forms on a BGR descriptor {OPK_FRAMES_BGR, n, width, height, {frames_dev}, {step}, {0}}.
 *
 * ONE DEFINITION: with NV12 / I420 frames every `_fmt` function gives, bit for bit, what it gives
 * on the BGR frames opk_frames_to_bgr makes of them -- the kernels convert what they read, no BGR
 * copy is written.  In particular taps outside the image contribute BGR (0,0,0), not YUV (0,0,0).
 *
 * The conversion is the arithmetic of OpenCV's cvtColor(COLOR_YUV2BGR_NV12 / _I420): BT.601
 * limited range in 20-bit fixed point; each 2x2 block of luma pixels shares one (U, V) pair
 * (nearest chroma, no interpolation).  In int32, `>>` arithmetic:
 *      y = max(0, Y - 16) * 1220542;   u = U - 128;   v = V - 128
 *      B = clamp((y + (1 << 19) + 2116026 * u)               >> 20, 0, 255)
 *      G = clamp((y + (1 << 19) -  852492 * v - 409993 * u)  >> 20, 0, 255)
 *      R = clamp((y + (1 << 19) + 1673527 * v)               >> 20, 0, 255)
 *
 * plane / step / frame_bytes are per plane, so the decoder's surfaces (Y and UV of one frame
 * adjacent, frames one surface apart) and plane-major batches are both described without a copy.
 * The descriptor is read during the call only (a pipeline that needs the frames later keeps a
 * copy of it); the planes follow the buffer rules of the pointer-taking form, the frame-lifetime
 * rule of opk_pose_attach_extractor included: it holds for EVERY plane.
 * OPK_ERR_ARG, before any device work: an unknown format; n < 0; a step shorter than its row; for
 * NV12 / I420 an odd width or height, a NULL plane the format needs (n > 0), and I420 chroma
 * planes with different steps.  n == 0 succeeds without device work where the pointer-taking form
 * does. */
#define OPK_FRAMES_BGR  0   /* plane[0]: [height][step[0]] packed BGR                      */
#define OPK_FRAMES_NV12 1   /* plane[0]: Y [height][step[0]]; plane[1]: UV pairs, U first,  */
                            /*           [height/2][step[1]]                                */
#define OPK_FRAMES_I420 2   /* plane[0]: Y; plane[1]: U, plane[2]: V, [height/2][step[1|2]] */
typedef struct opk_frames {
    int format, n, width, height;
    const uint8_t* plane[3];     /* device pointers of frame 0                              */
    size_t step[3];              /* row bytes; 0 = tight (w*3 | w | w (NV12) | w/2 (I420))  */
    size_t frame_bytes[3];       /* bytes from frame f to f+1 of that plane; 0 = step*rows  */
} opk_frames;
/* NV12 / I420 frames -> dst_dev BGR uint8 [n][height][dst_step] (dst_step 0 = width*3; only
 * width*3 bytes of a row are written), enqueued on the context's stream.  BGR frames are
 * OPK_ERR_ARG: there is nothing to convert. */
int opk_frames_to_bgr(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, const opk_frames* frames);
int opk_cvmat_to_input_fmt(opk_ctx* ctx, float* input_dev, const opk_frames* frames, double scale,
                           int net_w, int net_h, int normalize);

/* ---- Frames out as the encoders take them: the other direction, BGR -> NV12 / I420.
 *
 * The conversion is the arithmetic of OpenCV's cvtColor(COLOR_BGR2YUV_I420): BT.601 limited range
 * in 20-bit fixed point.  In int32, `>>` arithmetic:
 *      Y = (269484*R + 528482*G + 102760*B + (1<<19) + (16<<20))   >> 20    every pixel
 *      U = (-155188*R - 305135*G + 460324*B + (1<<19) + (128<<20)) >> 20    of the block's top-left
 *      V = (460324*R - 385875*G -  74448*B + (1<<19) + (128<<20))  >> 20    pixel (even x, even y);
 *                                                                           no averaging
 * NV12 is the same U and V, interleaved with U first (OpenCV's converter has no two-plane target:
 * for NV12 this text is the whole definition).  For every (B, G, R) each sum is non-negative and
 * below 2^31, Y lies in [16, 235] and U, V in [16, 240]: there is no clamp.  Black gives (Y, U, V)
 * = (16, 128, 128), white (235, 128, 128), blue (41, 240, 110), green (145, 54, 34), red
 * (82, 90, 240).
 *
 * ONE DEFINITION: with an NV12 / I420 destination every `_to` function below writes, bit for bit,
 * opk_bgr_to_frames of the bytes its BGR-out twin writes for the same arguments -- the render
 * converts in its store epilogue and writes no BGR image; with a BGR destination it writes exactly
 * the twin's bytes.  Only the samples are written: row padding and the bytes between frames keep
 * their values.
 *
 * opk_frames_out is opk_frames with writable planes and the same defaults for 0; width, height are
 * the drawn images' out_w, out_h.  OPK_ERR_ARG, before any device work: every descriptor error of
 * opk_frames; n differing from the source's; destination planes that overlap each other, another
 * frame of themselves, or the source frames (one byte range per plane and frame, from its first
 * sample to its last). */
typedef struct opk_frames_out {
    int format, n, width, height;
    uint8_t* plane[3];
    size_t step[3];
    size_t frame_bytes[3];
} opk_frames_out;
/* BGR frames -> NV12 / I420, the inverse direction of opk_frames_to_bgr, enqueued on the context's
 * stream.  A non-BGR source, a BGR destination and a destination of another width or height are
 * OPK_ERR_ARG; n == 0 succeeds without device work. */
int opk_bgr_to_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* bgr_src);

/* Kernel-variant switches (no reference counterpart; A/B tests and tuning only): key = one of
 * "CONV3_SMALL", "CONV3_W16", "CONV3_PERSIST", "CONV3_WIDE", "CONV3P_ASMR", "CONV3P_WIDE",
 * "CONV3P_PRIO", "CONV3W", "CONV1_TILE", "CONV1_N64W16", "CONV1_FUSED", "CONV3S_MAX", "LK_WAVE",
 * "TRI_GROUP" and the others named below and at their readers (opk::dev_switch);
 * reset != 0 removes the key (back to the product default).  Process-wide; the environment is
 * never consulted.
 * When a net reads them.  A decision switch -- one that chooses which kernel runs a conv, on which
 * tile, fused with what, on how many compute units: everything the host-side conv planner and the
 * net's shape planner read, plus "GRID_CUS" and "EPI_MAX" -- is read when a net plans an input
 * shape (its first forward, prepare or select_output of that shape) and holds for that shape's
 * plan: later forwards of the shape replay the planned launches.  A new net, opk_net_set_conv,
 * opk_net_set_precision, opk_net_set_precision_schedule and opk_net_set_small_batch plan again;
 * setting a decision switch does not, so set it before the net first sees the shape.
 * opk_net_conv_plan and opk_net_conv_kernels plan afresh on every call.  The flags with which a
 * launcher picks among instantiations of the planned kernel ("BUFST", "W8_NBX", "CONV3W" = 2,
 * "CONV3_WIDE", "CONV3P_PRIO", "CONV3P_ASMR", "CONV3P_WIDE", "HEAD_PERSIST", "CONV_IMAGE_WIDE",
 * "CONV_IMAGE_STAGE") and "LAUNCH_LOG" are read on every forward. */
int opk_dev_set(const char* key, int value, int reset);

/* ---- Net: replaces op::Net / op::NetCaffe (include/openpose/net/net.hpp:8-18,
 *      netCaffe.hpp:12-13).  prototxt: a Caffe prototxt path, or one of the reference's networks
 *      generated in the library: "builtin:BODY_25", "builtin:COCO_18", "builtin:MPI_15",
 *      "builtin:MPI_15_4", "builtin:HAND", "builtin:FACE" (models/.../pose_deploy*.prototxt).
 *      Supported layers: Convolution 3x3/pad 1, 7x7/pad 3, 1x1; ReLU/PReLU in place after a conv;
 *      MaxPool 2x2/2; channel Concat; the output blob is a Concat or a conv's top.  Any output
 *      count, except for the conv that reads the image: at most 64 outputs, a multiple of 4
 *      (refused at creation otherwise, with the layer's name in opk_last_error). */
typedef struct opk_net opk_net;
/* caffemodel (or NULL): trained weights, loaded as caffe::Net::CopyTrainedLayersFrom does
 * (netCaffe.cpp:163-185): every conv whose name is in the file gets its weights, bias and the
 * slopes of its PReLU layer, shapes checked; file layers the net lacks are ignored.  Convs not in
 * the file must be set with opk_net_set_conv before a forward. */
int opk_net_create(opk_ctx* ctx, const char* prototxt, const char* caffemodel, opk_net** out);
int opk_net_load_caffemodel(opk_net* net, const char* caffemodel, int* convs_loaded);
/* Host utility (no device): blob `index` of `layer` in a .caffemodel; shape gets <= 8 dims
 * (legacy 4-D shapes as stored), data (may be NULL) the float values. */
int opk_caffemodel_blob(const char* caffemodel, const char* layer, int index, float* data,
                        size_t capacity, int64_t* shape, int* ndim);
int opk_net_destroy(opk_net* net);
int opk_net_num_convs(opk_net* net);
/* name buffer >= 64 bytes; act: 0 none, 1 ReLU, 2 PReLU */
int opk_net_conv_info(opk_net* net, int index, char* name, int* cin, int* cout, int* kernel,
                      int* act);
/* Caffe layouts: weights [cout][cin][k][k], bias [cout], slope [cout] (NULL unless PReLU) */
int opk_net_set_conv(opk_net* net, const char* name, const float* weights_host,
                     const float* bias_host, const float* slope_host);
/* input NCHW fp32 on device: [n][3][h][w] (the net input blob, netCaffe.cpp:230-247) */
int opk_net_forward(opk_net* net, const float* input_dev, int n, int h, int w);
/* useful (unpadded) convolution FLOPs of one frame of h x w (2 * MACs, all conv layers) */
int opk_net_flops_per_frame(opk_net* net, int h, int w, double* flops);
/* Arithmetic of the forward (no reference counterpart: Caffe's forward is fp32).
 * OPK_PRECISION_FP16 (default): fp16 weights and stored activations, fp32 MFMA accumulation, the
 *   tuned fused kernels -- net output within rel-L2 ~2.5e-3 of fp32 on random He-initialised
 *   BODY_25 nets.
 * OPK_PRECISION_SPLIT: every weight and activation held as an fp16 hi/lo pair (x = hi + lo to
 *   ~22 bits; each layer's weights scaled by a power of two so that w_lo stays a normal fp16
 *   number), three MFMA passes per conv (x_hi w_hi + x_lo w_hi + x_hi w_lo, each product exact in
 *   fp32): fp32-level results (parity mode: as close to the exact convolution as an fp32 CPU
 *   implementation is) at 3x the MFMA work and 2x the activation bytes -- the 512-position
 *   persistent 8-wave kernel's split instantiation for every 96/128/256/512-channel 3x3 layer,
 *   conv_image's for the first conv, the generic kernel for the rest; no conv1 / head / pool
 *   fusion.  Re-plans the net's shapes; loaded weights are kept. */
#define OPK_PRECISION_FP16 0
#define OPK_PRECISION_SPLIT 1
int opk_net_set_precision(opk_net* net, int precision);   /* the uniform schedule */
/* Per-layer precision: one OPK_PRECISION_FP16 / OPK_PRECISION_SPLIT per conv, in
 * opk_net_conv_info order.  An fp16 conv reads the hi image of whatever it reads and writes hi
 * only; a split conv reads hi and lo and writes both.  A buffer has a lo twin iff a split conv (or
 * a pool fed by one) writes part of it; the lo channels under an fp16 writer stay zero.  A split
 * conv whose whole source was written by fp16 convs ("hi-only") runs two products per chunk
 * (x_hi w_lo + x_hi w_hi) on the hi-only instantiations of the generic kernel (3x3 and 1x1 tiles,
 * the small-batch 3x3 tiles; launch-log names ending ",split,xhi>") and reads no twin; where the
 * kernel that runs it has none (7x7, the persistent 8-wave kernel, a pooled epilogue, a fused head
 * pair) it runs the three-product kernel over a zero twin -- equal values.  The conv1 fusion needs
 * both of its convs fp16; a head pair runs fused only with equal precisions; a pool follows its
 * input.  Uniform schedules plan, launch and compute exactly as opk_net_set_precision.
 * count != opk_net_num_convs or any other value: OPK_ERR_ARG (the message names the index) and the
 * schedule in force stays.  Re-packs the convs whose precision changes and re-plans the shapes;
 * loaded weights are kept. */
int opk_net_set_precision_schedule(opk_net* net, const int* precisions, int count);
int opk_net_conv_precision(opk_net* net, int index);   /* -1 for NULL or a bad index */
/* Small-batch mode (no reference counterpart).  The default planning tiles every 3x3 and 7x7 conv
 * for the large batches of opk_pose_submit (256 or 512 positions x 64..128 outputs): a forward of
 * one frame, as op::PoseExtractorCaffe::forwardPass runs it, or of a few face / hand crops, leaves
 * most compute units idle.
 * 0 (default): today's planning.  1: 3x3 layers (any net) and 7x7 layers (the COCO / MPI / face /
 * hand stages) that would not fill the chip run on conv3s tiles; the 1x1 layers are planned as
 * without the mode.  Results are bit-identical either way.  Re-plans the net's shapes. */
int opk_net_set_small_batch(opk_net* net, int enable);   /* other values: OPK_ERR_ARG */
int opk_net_small_batch(opk_net* net);                    /* 0 / 1, -1 for NULL */
/* Host-only (works on a device -1 context): the conv geometry the planner picks for conv `index`
 * (opk_net_conv_info order) of an n x h x w forward on a chip of `cus` compute units: the GEMM
 * tile bm positions x bn outputs and `workgroups`, the tiles of the frames' h x (w + 2) positions
 * times the n-blocks (the launched grid also covers border rows; persistent kernels launch at
 * most `cus`).  The image conv has no GEMM tile and reports zeros.  Any output may be NULL. */
int opk_net_conv_plan(opk_net* net, int index, int n, int h, int w, int cus,
                      int* bm, int* bn, int* workgroups, int* small /* 1: conv3s */);
/* Host-only, the same shape arguments: which kernels such a forward launches for conv `index`, one
 * "<kernel>\n" line per launch in launch order, with the buffer convention of opk_net_launch_log.
 * A line is the launch log's kernel name up to the template arguments the planner fixes: the
 * whole instantiation for conv3_kernel and conv3s_kernel, "conv3w8_kernel<BN,NB,POOL",
 * "conv3w_kernel<BN" and "conv3p_kernel<BN" for the persistent kernels (the launch log's name
 * starts with it).  A conv split into frame runs gives one line per run; a conv inside
 * conv1_fused_kernel or conv_head_kernel gives that kernel's bare name on the unit's first conv
 * and no line on the others; the image conv outside the fused unit gives conv_image_kernel.  The
 * launchers take the kernel from the same plan, so the log of a real forward cannot differ. */
int opk_net_conv_kernels(opk_net* net, int index, int n, int h, int w, int cus,
                         char* buf, size_t size, size_t* needed);
/* Forward timing (measurement hook, no reference counterpart): while enabled every forward is
 * bracketed by HIP events on the context stream; read waits for them and returns the number of
 * forwards since the last read and their summed device time in milliseconds. */
int opk_net_set_timing(opk_net* net, int enable);
int opk_net_read_timing(opk_net* net, int* forwards, double* total_ms);
/* device pointer + NCHW shape of the last forward's net_output blob.  Valid right after
 * opk_net_create, as NetCaffe::getOutputBlobArray is (poseExtractorCaffe.cpp:94-95 takes it once,
 * before any forward, and keeps it): before the first forward *output_dev is NULL and shape is
 * {0, out_channels, 0, 0}.  The buffer of one input shape is stable across direct forwards of
 * that shape (the values are the latest forward's).  A net driven by an opk_pose pipeline
 * alternates between two output buffers per input shape (batch i+1's nets write the one batch i's
 * post-processing does not read), so re-query the pointer after each forward.  A forward that
 * writes a buffer a pipeline's post-processing still reads -- including a direct opk_net_forward
 * between opk_pose_submit and opk_pose_collect -- waits for that post-processing first. */
int opk_net_output(opk_net* net, float** output_dev, int shape[4]);
/* Inspection (caffe::Net::blob_by_name, which NetCaffe does not expose; used by the per-layer
 * parity tests): frames [frame0, frame0 + nframes) of the named top of the last forward -- a
 * conv, pool or concat top, or net_output -- converted from its padded NHWC fp16 buffer (the fp32
 * output for net_output) to fp32 NCHW host memory [nframes][channels][h][w]; host_out NULL:
 * shape only.  Synchronises the context stream.  Blobs that fused kernels keep on chip
 * (conv1_1 / conv1_2 with the fused first layers, a pooled conv's un-pooled output, Mconv6 of a
 * fused head pair) fail with the "kept on chip" message. */
int opk_net_blob(opk_net* net, const char* name, int frame0, int nframes, float* host_out,
                 int shape[4]);
/* The same blob as stored: the hi image and its lo twin, each fp32 NCHW [nframes][channels][h][w]
 * (opk_net_blob returns hi + lo where the buffer has a twin, else hi).  A buffer without a twin
 * (no split writer): lo is zeros and *has_lo = 0.  net_output: hi is the fp32 value.  Either
 * plane pointer may be NULL; fails for the same "kept on chip" blobs as opk_net_blob. */
int opk_net_blob_planes(opk_net* net, const char* name, int frame0, int nframes, float* hi_host,
                        float* lo_host, int shape[4], int* has_lo);
/* Kernels launched by the last forward run while the dev switch LAUNCH_LOG was 1, one
 * "<layer>\t<kernel instantiation>\n" line per launch.  *needed = bytes incl. the NUL; the text
 * is copied when size >= *needed. */
int opk_net_launch_log(opk_net* net, char* buf, size_t size, size_t* needed);
/* The same log outside a net forward (tests: which route a launcher took).  _begin attaches an
 * empty log owned by the library to the calling thread; every launch that thread makes until _end
 * adds its line (the layer is empty outside a forward; a forward run with LAUNCH_LOG 1 logs to the
 * net's own log and hands this one back afterwards).  _end detaches it and returns its lines with
 * the buffer convention above; it may be called again to fetch the text. */
int opk_launch_log_begin(void);
int opk_launch_log_end(char* buf, size_t size, size_t* needed);

/* ---- Pose extractor: replaces op::PoseExtractorCaffe::forwardPass
 *      (src/openpose/pose/poseExtractorCaffe.cpp:200-334) for a batch of frames:
 *      net -> resizeAndMerge -> NMS -> connector, one result set per frame. */
typedef struct opk_pose opk_pose;
/* PoseProperty (enumClasses.hpp:32-40) */
#define OPK_PROP_NMS_THRESHOLD 0
#define OPK_PROP_INTER_MIN_ABOVE_THRESHOLD 1
#define OPK_PROP_INTER_THRESHOLD 2
#define OPK_PROP_MIN_SUBSET_CNT 3
#define OPK_PROP_MIN_SUBSET_SCORE 4
int opk_pose_create(opk_ctx* ctx, opk_net* net /* may be NULL: net output injected */,
                    int maximize_positives, opk_pose** out);
/* any pose model (the net output / injected heat maps carry its heat_channels) and connector
 * semantics; opk_pose_create = (BODY_25, OPK_CONNECT_CPU).  OPK_CONNECT_CPU with a model the
 * reference's CPU connector rejects fails with OPK_ERR_UNSUPPORTED. */
int opk_pose_create_model(opk_ctx* ctx, opk_net* net, int pose_model, int maximize_positives,
                          int semantics, opk_pose** out);
/* A pose uses its net until it is destroyed (its forwards, and the net's record of the
 * post-processing still reading each output buffer): destroy the pose before the net, as the
 * reference's PoseExtractorCaffe owns its net. */
int opk_pose_destroy(opk_pose* pose);
int opk_pose_set_property(opk_pose* pose, int property, double value);
/* heat-map semantics of the pipeline's resize + NMS (OPK_MAPS_CPU, the default, or OPK_MAPS_CUDA:
 * what the reference's CUDA build computes, see opk_nms_semantics); the lazy heat maps, the PAF
 * samples and opk_pose_heatmaps follow it.  Multi-scale with OPK_MAPS_CUDA needs the raw-frame
 * path (opk_pose_submit_frames), which knows scaleInputToNetInputs. */
int opk_pose_set_map_semantics(opk_pose* pose, int semantics);
/* --upsampling_ratio (include/openpose/flags.hpp:136; PoseExtractorCaffe's upsamplingRatio):
 * heat maps of round((out_h * ratio - 1)) + 1 rows (likewise columns) of the scale-0 net output,
 * resizeAndMergeCaffe.cpp:77-81, instead of the net input size; scaleNetToOutput then uses
 * mNetOutputSize = round(ratio / 8 x net input size) (poseExtractorCaffe.cpp:281-310).  ratio <= 0
 * (the default) = the net's decrease factor (8; 4 for BODY_19_X2).  CPU map semantics; the CUDA
 * build's resize accepts x8 only for one source (resizeAndMergeBase.cu) and so does OPK_MAPS_CUDA. */
int opk_pose_set_upsampling_ratio(opk_pose* pose, float ratio);
/* frames: [n][3][net_h][net_w] device fp32; producer_w/h: original frame size (for
 * scaleNetToOutput, poseExtractorCaffe.cpp:306-310) */
int opk_pose_forward(opk_pose* pose, const float* frames_dev, int n, int net_h, int net_w,
                     int producer_w, int producer_h);
/* heat-map injection (poseNetOutput path, poseExtractorCaffe.cpp:249-262): net output on device
 * [n][heat_channels][h][w] (78 for BODY_25, 439 for BODY_135); net_h/net_w = the net input size
 * it corresponds to */
int opk_pose_forward_net_output(opk_pose* pose, const float* net_output_dev, int n, int out_h,
                                int out_w, int net_h, int net_w, int producer_w, int producer_h);
/* Pipelined use (the reference's producer/worker/consumer threads, wrapperAuxiliary.hpp, on one
 * GPU): submit enqueues a batch's device work (net, NMS, PAF scores) and returns; collect waits
 * for the OLDEST submitted batch, assembles its people on the host and makes it the batch the
 * result accessors below refer to.  At most two batches in flight: submit(i+1) then collect(i)
 * overlaps the host assembly of batch i with the device work of batch i+1.  opk_pose_forward* =
 * submit + collect.  *frames (may be NULL) receives the collected batch's frame count.
 * Streams: the frames / net inputs / injected net output are read after the work queued on the
 * context stream before the submit.  When the pipeline runs its own net, a batch's
 * post-processing (overlay add, NMS, PAF scores) runs on a side stream after the batch's nets, so
 * work queued on the context stream after the submit is NOT ordered before it: keep the overlay
 * unchanged until collect (or opk_sync); forwards of the same net are ordered after it by the
 * net (opk_net_output).  The injection path stays on the context stream. */
int opk_pose_submit(opk_pose* pose, const float* frames_dev, int n, int net_h, int net_w,
                    int producer_w, int producer_h);
int opk_pose_submit_net_output(opk_pose* pose, const float* net_output_dev, int n, int out_h,
                               int out_w, int net_h, int net_w, int producer_w, int producer_h);
int opk_pose_collect(opk_pose* pose, int* frames);
/* Multi-scale (--scale_number > 1; poseExtractorCaffe.cpp:240-245 runs the net once per scale,
 * resizeAndMergeCpu averages the x8 resizes of every scale's output, resizeAndMergeBase.cpp:55-106):
 * frames_dev[i] = [n][3][net_hw[2i]][net_hw[2i+1]] net input of scale i (the reference's
 * inputNetData[i]); scale 0 sets the heat-map size and scaleNetToOutput.  1..8 scales. */
int opk_pose_submit_multi(opk_pose* pose, const float* const* frames_dev, const int* net_hw,
                          int num_scales, int n, int producer_w, int producer_h);
int opk_pose_forward_multi(opk_pose* pose, const float* const* frames_dev, const int* net_hw,
                           int num_scales, int n, int producer_w, int producer_h);
/* Raw frames: the whole per-frame path of the reference's Wrapper workers
 * (WScaleAndSizeExtractor -> WCvMatToOpInput -> WPoseExtractorNet, wrapperAuxiliary.hpp):
 * frames_dev = n BGR uint8 frames [height][step bytes] on device (step 0 = width*3), prepared
 * on the GPU for every scale of opk_pose_set_input (default: -1x368, dynamic 1, one scale, gap
 * 0.25 -- the reference's flag defaults), then one net pass per scale and the merged
 * post-processing.  Keypoints are in frame pixels (scaleNetToOutput for a frame-sized output). */
int opk_pose_set_input(opk_pose* pose, int net_w, int net_h, float dynamic_behavior,
                       int scale_number, double scale_gap);
int opk_pose_submit_frames(opk_pose* pose, const uint8_t* frames_dev, int n, int width,
                           int height, size_t step);
int opk_pose_forward_frames(opk_pose* pose, const uint8_t* frames_dev, int n, int width,
                            int height, size_t step);
/* The same on an opk_frames descriptor (BGR, NV12 or I420; see opk_frames).  The pipeline keeps a
 * copy of the descriptor with the batch, not a pointer to it. */
int opk_pose_submit_frames_fmt(opk_pose* pose, const opk_frames* frames);
int opk_pose_forward_frames_fmt(opk_pose* pose, const opk_frames* frames);
/* net input of scale i prepared by the last opk_pose_submit_frames ([n][3][net_h][net_w]) */
int opk_pose_net_input(opk_pose* pose, int scale, const float** input_dev, int* net_w,
                       int* net_h);
int opk_pose_pending(opk_pose* pose);   /* batches in flight, -1 for NULL */
/* optional additive overlay on the net output before resize (synthetic-people workloads):
 * [n][78][out_h][out_w] device fp32, NULL to disable.  With a pipeline that runs its own net the
 * overlay is read by the post-processing stream after the batch's nets: rewrite it only after the
 * batch is collected (or after opk_sync). */
int opk_pose_set_overlay(opk_pose* pose, const float* overlay_dev);
int opk_pose_num_people(opk_pose* pose, int frame);
/* keypoints_host [max_people][parts][3], scores_host [max_people] of one collected frame */
int opk_pose_keypoints(opk_pose* pose, int frame, float* keypoints_host, float* scores_host,
                       int max_people);
/* Post-processing timing (measurement hook, no reference counterpart): while enabled the device
 * work of every submitted batch after its net forward (overlay add, NMS, PAF integrals) is
 * bracketed by HIP events on the stream it runs on -- the pipeline's post-processing stream when
 * it runs its own net (batch i's post-processing then shares the GPU with batch i+1's nets, so
 * the span includes that time-sharing), the context stream on the injection path; read waits for
 * them and returns the number of batches since the last read and their summed device time in
 * milliseconds. */
int opk_pose_set_timing(opk_pose* pose, int enable);
int opk_pose_read_timing(opk_pose* pose, int* batches, double* total_ms);
/* Host-side collect timing (measurement hook, no reference counterpart): for the collects since
 * the last read, their number and the summed milliseconds spent waiting for the batches' device
 * results and assembling their people; *workers = the assembly threads (at most 16 and at most
 * the CPUs of the process's affinity mask).  Any pointer may be NULL. */
int opk_pose_read_collect_times(opk_pose* pose, int* collects, double* wait_ms, double* assembly_ms,
                                int* workers);
/* Every frame of the last collected batch as one packed host record (the result the reference's
 * WQueueOrderer re-sequences, wQueueOrderer.hpp:62-141): for each frame f in order,
 *   [people_f, keypoints_f (people_f x parts x 3), scores_f (people_f)]  (all float).
 * *used receives the floats needed; with capacity < *used nothing is written and the call fails
 * with OPK_ERR_ARG (records may be NULL to query the size). */
int opk_pose_records(opk_pose* pose, float* records_host, size_t capacity, size_t* used);
/* device pointers of the last forward's heatmaps [n][heat_channels][H][W] and peaks
 * [n][parts][128][3].
 * The pipeline evaluates heat-map values lazily from the net output (NMS and PAF scoring compute
 * the resized values they touch, bit-identical to resizeAndMerge); opk_pose_heatmaps writes the
 * full stack on first request after a collect, while no later batch is in flight.  With
 * opk_pose_forward_net_output the net output buffer must stay unchanged until then. */
int opk_pose_heatmaps(opk_pose* pose, float** heat_dev, int shape[4]);
/* shape of the last collected batch's heat maps (spHeatMapsBlob->shape(), poseExtractorCaffe.cpp:
 * 651-663) without writing them */
int opk_pose_heatmap_size(opk_pose* pose, int shape[4]);
int opk_pose_peaks(opk_pose* pose, float** peaks_dev, int shape[4]);
float opk_pose_scale_net_to_output(opk_pose* pose);
/* PoseExtractorNet::getHeatMapsCopy (src/openpose/pose/poseExtractorNet.cpp:106-244) for every
 * frame of the last collected batch: types = OPK_HEATMAP_* bits (copied in the order parts,
 * background, PAFs, as --heatmaps_add_parts/_bkg/_PAFs), scale_mode = op::ScaleMode
 * (include/openpose/core/enumClasses.hpp:6-17; --heatmaps_scale: 5 PlusMinusOne, 3 ZeroToOne,
 * 7 UnsignedChar, 8 NoScale).  dst_dev [n][channels][H][W] device, or NULL to get the shape. */
#define OPK_HEATMAP_PARTS 1
#define OPK_HEATMAP_BACKGROUND 2
#define OPK_HEATMAP_PAFS 4
int opk_pose_heatmaps_copy(opk_pose* pose, int types, int scale_mode, float* dst_dev,
                           int shape[4]);
/* The same values for frames frame0 .. frame0 + nframes - 1 of the collected batch (nframes -1: to
 * the batch's end), written straight from the net output: one kernel evaluates the resize / merge
 * (1..8 sources, either map semantics, any upsampling ratio), the channel selection and the
 * scaling, so the full-resolution stack of opk_pose_heatmaps is neither allocated nor read.
 * dst_type OPK_F32: bit for bit opk_pose_heatmaps_copy's values.  OPK_U8, ScaleMode UnsignedChar
 * only (any other mode: OPK_ERR_ARG): min(value, 255) of those floats, which are non-negative
 * integers (the PAF mapping t * 128.5 + 128.5 reaches 256 and 257 at t = 1; they saturate).
 * dst_dev [nframes][channels][H][W] device, or NULL to get the shape.  Checked in this order:
 * the arguments (types, mode, type; frame0 < 0, or nframes neither positive nor -1: a range no
 * batch holds), OPK_ERR_ARG; then opk_pose_heatmaps' preconditions -- a collected batch and no
 * later batch in flight -- OPK_ERR_STATE; then the range against the batch, OPK_ERR_ARG.
 * Complete at return. */
int opk_pose_heatmaps_copy_range(opk_pose* pose, int types, int scale_mode, int frame0, int nframes,
                                 void* dst_dev, int dst_type, int shape[4]);
/* PoseExtractorNet::getCandidatesCopy (poseExtractorNet.cpp:246-282) of one collected frame:
 * candidates_host [parts][127][3] (x, y in output pixels = net pixels * scaleNetToOutput, score),
 * counts_host [parts]; either may be NULL. */
int opk_pose_candidates(opk_pose* pose, int frame, float* candidates_host, int* counts_host);


/* ---- face / hand keypoints -------------------------------------------------------------------
 * op::FaceDetector::detectFaces (include/openpose/face/faceDetector.hpp:10-27,
 * src/openpose/face/faceDetector.cpp:122-139) and op::HandDetector::detectHands
 * (include/openpose/hand/handDetector.hpp:13-45, src/openpose/hand/handDetector.cpp:135-160):
 * rectangles (x, y, width, height) from pose keypoints_host [people][parts][3] of pose_model;
 * rects_host face [people][4], hand [people][2 (left, right)][4].  A model without the detector's
 * body parts (e.g. CAR_12) fails with OPK_ERR_UNSUPPORTED, as poseBodyPartMapStringToKey errors. */
int opk_face_detect(int pose_model, const float* keypoints_host, int people, int parts,
                    float* rects_host);
int opk_hand_detect(int pose_model, const float* keypoints_host, int people, int parts,
                    float* rects_host);

/* op::FaceExtractorCaffe / op::HandExtractorCaffe (include/openpose/face/faceExtractorCaffe.hpp:
 * 14-45, include/openpose/hand/handExtractorCaffe.hpp:14-52): forwardPass(rectangles, inputData)
 * + getFaceKeypoints() / getHandKeypoints(), for every rectangle of a set of frames at once.  net:
 * the face (builtin:FACE, pose_deploy.prototxt of models/face) or hand (builtin:HAND) net;
 * net_w x net_h = --face_net_resolution / --hand_net_resolution (multiples of 16, default
 * 368x368). */
typedef struct opk_extractor opk_extractor;
#define OPK_EXTRACT_FACE 0
#define OPK_EXTRACT_HAND 1
/* A host-only context may create an extractor (and attach it to a pose extractor, for the
 * argument and state checks); it used to be refused here with OPK_ERR_ARG, now
 * opk_extractor_forward is what needs a device context (OPK_ERR_ARG there). */
int opk_extractor_create(opk_ctx* ctx, opk_net* net, int kind, int net_w, int net_h,
                         opk_extractor** out);
int opk_extractor_destroy(opk_extractor* ex);
/* hand only: --hand_scale_number / --hand_scale_range (HandExtractorNet, handExtractorNet.cpp) */
int opk_extractor_set_scales(opk_extractor* ex, int number, float range);
/* crops per net forward (default 32; batches run in power-of-two sizes) */
int opk_extractor_set_max_batch(opk_extractor* ex, int max_batch);
int opk_extractor_parts(opk_extractor* ex);   /* net output channels - 1; -1 for NULL */
/* per-person heat maps (--heatmaps_add_* with --face / --hand; FaceExtractorNet::getHeatMaps,
 * HandExtractorNet::getHeatMaps): scale_mode = op::ScaleMode of --heatmaps_scale (-1 off).  The
 * first `parts` channels of each rectangle's x8-resized crop output, mapped as
 * updateFaceHeatMapsForPerson / updateHandHeatMapsForPerson do (faceExtractorCaffe.cpp:42-75,
 * handExtractorCaffe.cpp:126-160): PlusMinusOne(FixedAspect) fastTruncate(v)*2-1, UnsignedChar
 * (float)positiveIntRound(fastTruncate(v)*255), any other mode fastTruncate(v).  With several hand
 * scales the last scale's maps are kept (the reference copies its blob after the last net run). */
int opk_extractor_set_heatmaps(opk_extractor* ex, int scale_mode);
/* after opk_extractor_forward: device pointer + shape {hands (1 face / 2 hand), people, parts, H,
 * W}; zeros for the rectangles the reference skips.  Valid until the next forward. */
int opk_extractor_heatmaps(opk_extractor* ex, const float** heatmaps_dev, int shape[5]);
/* frames_dev: BGR uint8 [nframes][height][step] on device (step 0: width*3); rects_host as
 * opk_face_detect / opk_hand_detect return them; frame_of_host [people] (NULL: frame 0).
 * keypoints_host: face [people][parts][3], hand [2][people][parts][3] (left hands first), in
 * frame pixels; zeros where the reference skips the rectangle (face: side <= 40; hand: side <= 1
 * or area <= 10).  A non-square rectangle fails with OPK_ERR_ARG as the reference errors. */
int opk_extractor_forward(opk_extractor* ex, const uint8_t* frames_dev, int nframes, int width,
                          int height, size_t step, const float* rects_host,
                          const int* frame_of_host, int people, float* keypoints_host);
int opk_extractor_forward_fmt(opk_extractor* ex, const opk_frames* frames, const float* rects_host,
                              const int* frame_of_host, int people, float* keypoints_host);
/* crops of the last forward (order: hand, person, scale; skipped rectangles have none): the 2x3
 * inverse map (frame <- crop) and the crop's net input [3][net_h][net_w] on device */
int opk_extractor_crop_count(opk_extractor* ex);
int opk_extractor_crop(opk_extractor* ex, int i, double* matrix_host, const float** input_dev);

/* ---- Face / hand stages inside the pose pipeline (the reference's --face --hand wiring:
 * WFaceDetector + WFaceExtractorNet and WHandDetector + WHandExtractorNet behind WPoseExtractor,
 * wrapperAuxiliary.hpp).  At most one face and one hand extractor per pose extractor.  The
 * extractor must be of the pose extractor's context and its net must not be the pose net
 * (OPK_ERR_ARG); the pose model must have the detector's body parts (OPK_ERR_UNSUPPORTED, as
 * opk_face_detect); a second extractor of a kind, and attaching or detaching with batches in
 * flight, are OPK_ERR_STATE.  An extractor destroyed while attached counts as detached from then on.
 * While one is attached the pipeline accepts the raw-frame path only (opk_pose_submit_frames,
 * opk_pose_forward_frames): every other submit / forward fails with OPK_ERR_STATE, because face /
 * hand extraction needs the frames.  opk_pose_collect then, after the host assembly of batch i,
 * builds each frame's rectangles from the batch's keypoints (opk_face_detect / opk_hand_detect of
 * what opk_pose_keypoints returns), concatenates them in frame order and runs the attached
 * extractors on batch i's frames, on the context stream -- behind the nets of batch i + 1 that an
 * earlier submit queued, so the device stays busy during assembly and table building.
 * Frame lifetime (beside the stream contract of opk_pose_submit): THE FRAME BUFFER OF A SUBMITTED
 * BATCH MUST STAY UNCHANGED UNTIL THAT BATCH IS COLLECTED.
 * (With an opk_frames descriptor that is every plane of it; the descriptor itself is copied at the
 * submit and may go away.)
 * The stage warps each net batch's crops right before its forward, so it holds at most max_batch
 * crops of net input whatever the number of people and frames (same kernel, tables and stream
 * order as opk_extractor_forward: the same values); after a stage run opk_extractor_crop returns
 * the matrix and a NULL input pointer. */
int opk_pose_attach_extractor(opk_pose* pose, opk_extractor* ex);
int opk_pose_detach_extractor(opk_pose* pose, int kind);   /* OPK_EXTRACT_* */
/* Results of the last collected batch, person order that of opk_pose_keypoints(frame):
 * rects_host face [people][4], hand [people][2 (left, right)][4]; keypoints_host face
 * [people'][70][3], hand [2][people'][21][3] (left hands first), people' = min(people, max_people);
 * zeros where the reference skips the rectangle.  OPK_ERR_STATE when no such extractor is attached
 * or nothing is collected since. */
int opk_pose_part_rectangles(opk_pose* pose, int kind, int frame, float* rects_host);
int opk_pose_part_keypoints(opk_pose* pose, int kind, int frame, float* keypoints_host,
                            int max_people);
/* Stage timing (measurement hook, modelled on opk_pose_read_collect_times): since the last read,
 * the collects that ran the stage, the crops they ran, the host milliseconds spent on rectangles,
 * crop validity and tables, and the milliseconds spent where the host can block on the device:
 * from the table upload (a copy that waits for the work queued ahead on the stream) through the
 * enqueue of every net batch (launches wait for room in the queue) to the end of the final
 * synchronisation.  host_ms + wait_ms is the stage's wall time but for the keypoint mapping.
 * Pointers may be NULL. */
int opk_pose_read_part_times(opk_pose* pose, int kind, int* batches, int* crops, double* host_ms,
                             double* wait_ms);

/* ---- Person ids across frames: op::PersonIdExtractor (--identification;
 * include/openpose/tracking/personIdExtractor.hpp:11-12, src/openpose/tracking/personIdExtractor.cpp:
 * 83-290, 429-476) on pyramidal Lucas-Kanade (src/openpose/tracking/pyramidalLK.cpp:272-368,
 * pyramidalLK.cu).  The reference's constructor throws ("buggy and not working yet",
 * personIdExtractor.cpp:416) and hands a 3-channel float image to code that indexes one channel, so
 * there is nothing to run it against: this text is the definition, on a single-channel image
 * defined here; parity with the reference is by restatement (tests/lk_cases.py) only.
 * op::PersonTracker (--tracking) is out of scope.
 * Everything is fp32 with every multiply and add rounded separately and correctly rounded division
 * and square root, unless integers are named.
 *
 * GREY IMAGE.  G = (1868*B + 9617*G + 4899*R + 8192) >> 14 of the BGR pixel, an integer in
 * [0, 255] taken as a float.  ONE DEFINITION: for NV12 / I420 frames it is the grey of the BGR pixel
 * opk_frames_to_bgr makes -- not the Y sample; no BGR copy is written.
 *
 * PYRAMID, `levels` = 1..3 levels, level 0 the grey image.  Level l+1 of a w x h level has
 * ((w+1)/2) x ((h+1)/2) pixels; pixel (x, y) is the sum of the taps 1 4 6 4 1 in x, then in y,
 * around (2x, 2y), times 1/256; an index outside the level is reflected without repeating the edge
 * (-1 -> 1, -2 -> 2, n -> n-2, again until it is inside; a length-1 axis always gives 0).  Level 1
 * is k / 2^8 with k < 2^16 and level 2 k / 2^16 with k < 2^24, every partial sum an integer below
 * 2^24: exact in fp32 in any order.  A fourth level is not, so levels > 3 is OPK_ERR_ARG.
 * Storage (opk_pyramid_layout): one record per frame -- level 0 uint8, level 1 uint16 (the k above),
 * level 2 float, each level [h][w] tight and starting on a 16-byte boundary of the record; 1.61 MB
 * per 1280x720 frame against 4.84 MB all in float.  opk_pyramid_level returns any level as fp32.
 *
 * ONE POINT (levels 3, patch 21): (x, y, status) in level-0 pixels, from pyramid I to pyramid J.
 *   A point whose status is not 0 is returned unchanged (pyramidalLK.cu:41).  A coordinate that is
 *   not finite or has |c| >= 2^24 gives status 3 and the point unchanged.  Otherwise
 *   pI = (x * 0.25f, y * 0.25f), pJ = pI, and for l = 2, 1, 0 with w, h the size of level l and
 *   xi = (int)pI.x, yi = (int)pI.y, xj = (int)pJ.x, yj = (int)pJ.y (toward zero; a value that is
 *   not inside (-2^30, 2^30), NaN included, counts as outside every level):
 *     gradient patch: if xi-11 < 0 || xi+11 >= w || yi-11 < 0 || yi+11 >= h every ix, iy is 0;
 *       otherwise for i, j in -10..10 (i the row):
 *       ix = (I[yi+i][xi+j+1] - I[yi+i][xi+j-1]) / 2,  iy = (I[yi+i+1][xi+j] - I[yi+i-1][xi+j]) / 2;
 *     time patch: if (xi, yi) +- 10 leaves I or (xj, yj) +- 10 leaves J every `it` is 0, otherwise
 *       it = J[yj+i][xj+j] - I[yi+i][xi+j];
 *     sxx = sum ix*ix, syy = sum iy*iy, sxy = sum ix*iy, sxt = sum ix*it, syt = sum iy*it, each
 *       accumulated sequentially from 0 in row-major order (i outer, j inner), product rounded, then
 *       added;
 *     den = sxx*syy - sxy*sxy; if |den| < 1e-9f the level's status is 3 and pJ stays, otherwise
 *       pJ.x += ((-1*syy)*sxt + sxy*syt) / den,  pJ.y += ((-1*sxx)*syt + sxt*sxy) / den;
 *     a non-zero level status becomes the point's status and stays; the later levels still run;
 *     after levels 2 and 1, pI and pJ are multiplied by 2.
 *   The result is (pJ, status).  Nothing is read before its bounds test.
 *
 * MATCHING (matchLKAndOPGreedy), opk_match_people: entries [n][parts][3] and people [m][parts][3]
 *   hold (x, y, status); a part is active for a pair when both statuses are 0.
 *   threshold = max(10.f, distance * (float)sqrt((double)(width*height)) / 960.f).
 *   Rounds until one assigns nobody: best = 0; for every person without an id, in order, and every
 *   entry not yet used, in ascending id order: d = sqrtf(dx*dx + dy*dy) of every active part (entry
 *   minus person), total = their sequential sum, inliers those with d < threshold, score =
 *   inliers / (float)active (no active part: the pair is skipped); if score == best && score >=
 *   inlier_ratio the pair joins the round's candidates, else if score > best && score >=
 *   inlier_ratio it becomes the only candidate and best = score.  The candidates are then taken by
 *   ascending total (a NaN total last); where the reference leaves the order open (unordered_map
 *   iteration, an unstable sort) equal totals go by the lower entry id, then the lower person index.
 *   A candidate whose entry is used is skipped; otherwise the person gets the entry's id -- also a
 *   person who got one earlier in the round -- and the entry is used.
 *   Afterwards every person still without an id gets next_id++, in person order.
 *
 * TRACKER.  State: next_id (from 0), the previous frame's pyramid, entries {id -> parts x (x, y,
 *   status), counter}.  Defaults (personIdExtractor.hpp:11-12): confidence 0.1, inlier ratio 0.5,
 *   distance 30, frames to delete 10.  Per frame, with its keypoints [people][parts][3] (x, y, score):
 *   1. capture: every person as (x, y, status), status 1 where score < confidence, else 0;
 *   2. the first frame: every person becomes an entry of its capture with id next_id++, counter 0;
 *   3. any later frame: every entry, in id order: if (counter++ > frames_to_delete) it is erased,
 *      otherwise all its points are propagated from the previous pyramid to this frame's;
 *   4. matching of the entries against the captures (on the first frame too);
 *   5. every person's entry (its id's) is replaced by its capture, counter 0.
 *   A frame without people still ages and propagates.  Frames of another size, or people of another
 *   part count, than the state holds are OPK_ERR_STATE until opk_tracker_reset. */
typedef struct opk_lk_point {
    int frame_i, frame_j;   /* pyramids I and J: records of the batch buffer, -1 = the carry record */
    float x, y;
    int status;
} opk_lk_point;
/* level sizes, byte offsets of the levels in a frame's record, and the record's bytes (any output
 * may be NULL; the arrays take `levels` entries) */
int opk_pyramid_layout(int width, int height, int levels, int* level_w, int* level_h,
                       size_t* level_offset, size_t* frame_bytes);
/* grey + pyramid of every frame (BGR, NV12, I420; any step; odd sizes for BGR) into pyramid_dev,
 * frames->n records of opk_pyramid_layout(frames->width, frames->height, levels); enqueued on the
 * context's stream */
int opk_pyramid_build(opk_ctx* ctx, void* pyramid_dev, const opk_frames* frames, int levels);
/* dst_dev float [n][level_h][level_w] = level `level` of n records (tests, debugging) */
int opk_pyramid_level(opk_ctx* ctx, float* dst_dev, const void* pyramid_dev, int n, int width,
                      int height, int levels, int level);
/* One launch over npoints records on the device, updated in place: frame_i / frame_j index the
 * n_frames records of pyramid_dev (3 levels of width x height), -1 the single record carry_dev (may
 * be NULL).  A record naming a frame outside them gets status 3 and is not followed.  Enqueued on
 * the context's stream. */
int opk_lk_points(opk_ctx* ctx, const void* pyramid_dev, int n_frames, const void* carry_dev,
                  int width, int height, opk_lk_point* points_dev, int npoints);
/* MATCHING above, a pure host function (no context): entry_ids_host strictly ascending;
 * ids_host [people]; *next_id is read and advanced. */
int opk_match_people(const float* entries_host, const long long* entry_ids_host, int n_entries,
                     const float* people_host, int people, int parts, float inlier_ratio,
                     float distance, int width, int height, long long* next_id,
                     long long* ids_host);

typedef struct opk_tracker opk_tracker;
int opk_tracker_create(opk_ctx* ctx, float confidence, float inlier_ratio, float distance,
                       int frames_to_delete, opk_tracker** out);
int opk_tracker_destroy(opk_tracker* t);
int opk_tracker_reset(opk_tracker* t);
/* frames->n frames in order; keypoints_host: their people one frame after the other
 * [sum(people_per_frame)][parts][3]; ids_host [sum(people_per_frame)].  Any number of calls: the
 * state carries over, and the ids equal those of the same frames given one at a time.  Between
 * calls only the last frame's pyramid is kept.  The fresh points of the whole batch -- frame f-1's
 * people into frame f, the carried frame's into frame 0 -- go in one launch; entries nobody
 * re-detected are propagated with one small launch per frame that has any.  Synchronous. */
int opk_tracker_update(opk_tracker* t, const opk_frames* frames, const float* keypoints_host,
                       const int* people_per_frame, int parts, long long* ids_host);
/* Measurement hook: while enabled the pyramid and LK launches are bracketed by HIP events; read
 * returns, since the last read, the updates, their device milliseconds, and the host milliseconds
 * of capture, bookkeeping and matching (the waits for the device excluded); device_bytes = the
 * pyramids, the carried frame and the point records held.  Pointers may be NULL. */
int opk_tracker_set_timing(opk_tracker* t, int enable);
int opk_tracker_read_times(opk_tracker* t, int* batches, double* pyramid_ms, double* lk_ms,
                           double* host_ms, size_t* device_bytes);
/* The tracker as a stage of the pose pipeline, under the rules of opk_pose_attach_extractor: the
 * tracker must be of the pose extractor's context (OPK_ERR_ARG); a second tracker, and attaching or
 * detaching with batches in flight, are OPK_ERR_STATE; a tracker destroyed while attached counts as
 * detached.  While attached the pipeline accepts the raw-frame path only (every other submit /
 * forward: OPK_ERR_STATE) and the frame-lifetime rule holds.  The pyramid of a batch is queued at its
 * submit, on the context stream; opk_pose_collect then, after the people assembly and the face /
 * hand stages, runs LK and the matching of the batch's frames (opk_tracker_update's steps on
 * opk_pose_keypoints' arrays) on the context stream -- behind the nets of the next batch that an
 * earlier submit queued. */
int opk_pose_attach_tracker(opk_pose* pose, opk_tracker* t);
int opk_pose_detach_tracker(opk_pose* pose);
/* ids of one collected frame, person order that of opk_pose_keypoints; OPK_ERR_STATE without a
 * tracker or a batch collected with it */
int opk_pose_person_ids(opk_pose* pose, int frame, long long* ids_host);
/* opk_tracker_read_times of the attached tracker */
int opk_pose_read_track_times(opk_pose* pose, int* batches, double* pyramid_ms, double* lk_ms,
                              double* host_ms);

/* ---- 3-D keypoints from a camera rig: op::PoseTriangulation::reconstructArray behind
 * op::WPoseTriangulation (--3d; include/openpose/3d/wPoseTriangulation.hpp:62-100,
 * src/openpose/3d/poseTriangulation.cpp:8-166, src/openpose/3d/poseTriangulationPrivate.cpp:11-33,
 * 119-226), the reference's default build: the USE_CERES refinement (poseTriangulationPrivate.cpp:
 * 228-290) is out of scope, as is the 3-D renderer; the calibration files and --frame_undistort
 * are the section after this one.
 * The reference takes the null vector of each point's matrix from OpenCV's cv::SVD; OpenCV is not
 * here, so this text is the definition -- a one-sided Jacobi of the form cv::SVD's JacobiSVDImpl_
 * has -- and parity with cv::SVD is by restatement only (tests/triangulate_cases.py, which is also
 * held against LAPACK's SVD: every float within 1 ulp, every decision equal).
 * Everything is fp64 unless named, with every multiply and add rounded separately and correctly
 * rounded division and square root.  A NaN is any NaN: payload and sign are not defined.
 *
 * RIG (opk_rig).  V views, 2 <= V <= 7 (the reference refuses a point seen by 8 or more,
 *   poseTriangulationPrivate.cpp:163-170); per view a 3x4 row-major double camera matrix P and an
 *   image size (w, h) with w, h > 0 and w*h an int.  V outside 2..7, a matrix entry that is not
 *   finite or a bad size is OPK_ERR_ARG.  min_views is >= 2 or negative; 0 and 1 are OPK_ERR_ARG
 *   (the PoseTriangulation constructor, poseTriangulation.cpp:168-182); negative means
 *   max(2, min(4, V-1)).
 *
 * INPUT.  Per time step and view one array [parts][3] of (x, y, score) in float -- person 0 of
 *   that view, as the reference indexes it -- and a `present` flag: whether the view has any person
 *   (its array is not empty).
 *
 * STEP RESULT.  Fewer than 2 present views: the empty array, status 0 (the reference's "not a 3-D
 *   problem").  Otherwise a part is valid in a view when the view is present and score > 0.35f &&
 *   x > 8 && x < w-8 && y > 8 && y < h-8 (isValidKeypoint): strict, in float against the int
 *   bounds converted to float, so NaN and infinities never get in.  A part is attempted when its
 *   valid views number >= the effective min_views.  No attempted part: status 0.  Otherwise status 1
 *   and the result is [parts][4], zeros but for the parts written below.
 *
 * ONE TRIANGULATION over a set S of views.  A is 2V x 4: rows 2i and 2i+1 are x_i*P_i[2] - P_i[0]
 *   and y_i*P_i[2] - P_i[1] for i in S (x_i, y_i the floats as doubles) and zero for a view outside
 *   S -- the shape is fixed and every sum gains exact zeros.  The null vector by cyclic one-sided
 *   Jacobi on the four columns: W[i] = the squared norm of column i, summed over the rows in order
 *   from 0; V = I; up to 30 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  For a pair
 *   (i, j): p = the sum over the rows k, in order from 0, of A[k][i]*A[k][j]; the pair is skipped
 *   when |p| <= DBL_EPSILON*sqrt(W[i]*W[j]); otherwise p *= 2, beta = W[i]-W[j], gamma =
 *   sqrt(p*p + beta*beta) and
 *     beta < 0:  delta = (gamma-beta)*0.5,  s = sqrt(delta/gamma),  c = p/(gamma*s*2);
 *     else:      c = sqrt((gamma+beta)/(gamma*2)),  s = p/(gamma*c*2)
 *   (products left to right); every row of both columns is rotated, t0 = c*a_i + s*a_j, t1 =
 *   c*a_j - s*a_i, W[i] and W[j] are summed again from the rotated entries, and the four rows of V
 *   get the same rotation.  A sweep without a rotation ends the loop.  The null vector v is the
 *   column of V with the smallest W, the lowest index among equals (found by `W[i] < smallest`).
 *   X = v / v[3], all four components divided.  The reprojection error is the sum over i in S, in
 *   view order from 0, of sqrt(dx*dx + dy*dy), divided by the size of S, where (u, v, w) = P_i X,
 *   each row the sum over k = 0..3 in order from 0, dx = u/w - x_i, dy = v/w - y_i.
 *
 * ONE POINT.  Triangulate over its valid views: error e.  When the valid views number >= 4 and
 *   e > 0.5*maxAcc, leave one out: best = e; for each valid view i in view order, triangulate
 *   without it, error e_i; if best > e_i && e_i < 0.9*e the subset becomes the best.  If one did,
 *   the point, its error and its dropped view (the rig's index of i) are that subset's.
 *   maxAcc = 25*sqrt(w0*h0/1310720.), w0*h0 the int product of view 0's size.
 *
 * ONE ARRAY OF A STEP.  total = the sum of the attempted parts' errors in part order from 0,
 *   divided by their count.  A part is written as (float)x, (float)y, (float)z, 1 when the three
 *   floats are finite && err < 5*total && err < maxAcc.  It follows that one NaN error makes total
 *   NaN and so rejects every part of that array (the status stays 1: the array is all zeros) --
 *   two identical cameras at the origin do that.
 *
 * opk_camera_matrix: out[3][4] = intrinsics[3][3] * extrinsics[3][4], the product
 *   cameraParameterReader.cpp:72 forms; each entry the sum over k = 0..2 in order from 0.
 * opk_triangulate_host: a pure host function (no context).  keypoints_host [steps][V][parts][3],
 *   present_host [steps][V] (0 / not 0); xyz_host [steps][parts][4] (zeros for status 0),
 *   status_host [steps]; optional errors_host [steps][parts] (-1 where the part was not
 *   attempted) and dropped_host [steps][parts] (the dropped view, or -1).
 * opk_triangulate: the same call on device buffers, enqueued on the context's stream: one launch
 *   over the points (8 lanes per point: lane 0 over all valid views, lane s without view s-1, the
 *   choice a shuffle minimum with the lowest view winning ties -- the sequential rule's choice)
 *   and one small launch for each array's total and acceptance, a sequential walk.  The rig is
 *   read on the host before the call returns.  Bit for bit opk_triangulate_host.
 * Both replace PoseTriangulation::reconstructArray for one kind of array; INTEGRATION.md. */
typedef struct opk_rig {
    int views;                      /* V */
    const double* camera_matrices;  /* [V][3][4] */
    const int* image_sizes;         /* [V][2]: width, height */
    int min_views;                  /* --3d_min_views: >= 2, or negative */
} opk_rig;
int opk_camera_matrix(const double* intrinsics, const double* extrinsics, double* out);
int opk_triangulate_host(const opk_rig* rig, int steps, int parts, const float* keypoints_host,
                         const int* present_host, float* xyz_host, int* status_host,
                         double* errors_host, int* dropped_host);
int opk_triangulate(opk_ctx* ctx, const opk_rig* rig, int steps, int parts,
                    const float* keypoints_dev, const int* present_dev, float* xyz_dev,
                    int* status_dev, double* errors_dev, int* dropped_dev);
/* The rig as a stage of the pose pipeline (WPoseTriangulation), under the attach rules of
 * opk_pose_attach_tracker: setting or clearing (rig NULL) with batches in flight is OPK_ERR_STATE;
 * the rig is copied.  While set, a batch of n frames is n / V time steps, frame t*V + v the view v
 * of step t: n not a multiple of V, or a frame size other than the rig's for that view, is
 * OPK_ERR_ARG at submit.  opk_pose_collect then, after the people assembly and the face / hand
 * stages, uploads person 0 of every frame (present: the frame has a person) for the body array
 * and, where extractors are attached, the face and both hand arrays, runs opk_triangulate once per
 * array kind on the context stream -- behind the nets of the next batch that an earlier submit
 * queued -- and downloads the results.
 * opk_pose_keypoints_3d: xyz_host [parts][4] of the kind (the model's parts, 70, 21, 21) and the
 * status of one step of the collected batch; every frame of the step carries these arrays
 * (wPoseTriangulation.hpp:94-100).  OPK_ERR_STATE without views, without a batch collected with
 * them, or for a face / hand kind whose extractor is not attached. */
#define OPK_3D_BODY 0
#define OPK_3D_FACE 1
#define OPK_3D_HAND_LEFT 2
#define OPK_3D_HAND_RIGHT 3
int opk_pose_set_views(opk_pose* pose, const opk_rig* rig);
int opk_pose_keypoints_3d(opk_pose* pose, int step, int kind, float* xyz_host, int* status);

/* ---- Undistorted rig frames and the calibration files: op::CameraParameterReader
 * (include/openpose/3d/cameraParameterReader.hpp; readParameters, src/openpose/3d/
 * cameraParameterReader.cpp:85-173, and undistort, :337-399, which the producer runs on every frame
 * under --frame_undistort, producer.cpp:115-119): cv::initUndistortRectifyMap(K, dist, I, K, size,
 * CV_16SC2) once per camera and cv::remap(INTER_LINEAR, constant border 0) per frame.  OpenCV is
 * not here, so this text is the definition -- OpenCV 4.2's scalar path with those arguments (R the
 * identity, the new camera matrix K itself) -- and parity with OpenCV is by restatement only
 * (tests/undistort_cases.py, which is also held against an evaluation without the row
 * accumulation in extended precision).  Every operation below is fp64 and rounded on its own.
 *
 * CAMERAS (opk_cameras).  V >= 1 views; per view intrinsics K[3][3] row-major, ncoef distortion
 *   coefficients, ncoef in {4, 5, 8, 12}, in the order k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (the
 *   absent ones are 0; view v's start at distortions[12 * v]), and an image size (w, h).
 *   OPK_ERR_ARG: V < 1, an entry that is not finite, any other ncoef, a singular K (the
 *   determinant below is 0) or a size <= 0.  ncoef = 14 (the tilted-sensor model) is
 *   OPK_ERR_UNSUPPORTED.
 *
 * THE MAP OF ONE CAMERA, m1 [h][w][2] int16 and m2 [h][w] uint16.
 *   ir = the inverse of K by the 3x3 closed form:
 *     det = K00*(K11*K22 - K12*K21) - K01*(K10*K22 - K12*K20) + K02*(K10*K21 - K11*K20), d = 1/det,
 *     ir[0] = (K11*K22 - K12*K21)*d   ir[1] = (K02*K21 - K01*K22)*d   ir[2] = (K01*K12 - K02*K11)*d
 *     ir[3] = (K12*K20 - K10*K22)*d   ir[4] = (K00*K22 - K02*K20)*d   ir[5] = (K02*K10 - K00*K12)*d
 *     ir[6] = (K10*K21 - K11*K20)*d   ir[7] = (K01*K20 - K00*K21)*d   ir[8] = (K00*K11 - K01*K10)*d
 *   With fx = K00, fy = K11, u0 = K02, v0 = K12, row i starts at _x = i*ir[1] + ir[2],
 *   _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8], and after each column _x += ir[0], _y += ir[3],
 *   _w += ir[6]: the accumulation along the row is part of the definition.  At column j
 *     w = 1/_w;  x = _x*w;  y = _y*w;  x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  _2xy = 2*x*y;
 *     kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2);
 *     xd = x*kr + p1*_2xy + p2*(r2 + 2*x2) + s1*r2 + s2*r2*r2;
 *     yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy + s3*r2 + s4*r2*r2;
 *     u = fx*xd + u0;  v = fy*yd + v0
 *   (sums and products left to right).  iu = round_half_even(u*32) and iv likewise, as int32; a
 *   product that is NaN or rounds outside the int32 range gives INT_MIN, as x86's conversion
 *   does.  m1[i][j] = ((short)(iu >> 5), (short)(iv >> 5)), the shift arithmetic and the short
 *   the low 16 bits; m2[i][j] = (uint16)((iv & 31)*32 + (iu & 31)).
 *
 * THE REMAP OF ONE FRAME, BGR uint8, constant border 0.  For the destination pixel (x, y):
 *   (sx, sy) = m1[y][x], f = m2[y][x], wt = T[f >> 5][f & 31] -- the 2x2 int16 weights of the
 *   bilinear fixed-point table of the frame warp (initInterTab2D(INTER_LINEAR, fixpt); sum 32768)
 *   -- and per channel
 *     D = (S(sy, sx)*wt00 + S(sy, sx+1)*wt01 + S(sy+1, sx)*wt10 + S(sy+1, sx+1)*wt11 + 16384) >> 15
 *   with S = 0 at any tap outside the frame: what remapBilinear computes on both of its paths.
 *   NV12 / I420 sources: the result is the remap of opk_frames_to_bgr(frames); every tap is
 *   converted as it is read and no BGR copy of the source is made.
 *
 * WHICH CAMERA.  Frame f uses view f % V, the rule of opk_pose_set_views.  The reference builds
 *   every camera's map from camera 0's intrinsics and distortion (cameraParameterReader.cpp:
 *   354-355); this interface takes each view's own: passing camera 0's for every view reproduces
 *   the reference.
 *
 * opk_undistort_maps_host: a pure host function (no context): the map of one view, m1_host
 *   [h][w][2], m2_host [h][w].
 * opk_undistort_frames: src (n frames of any format) -> dst (BGR, the same n and size), enqueued on
 *   the context's stream: kernels/undistort.hip, one launch per view over the view's frames.  The
 *   maps are built on the host and uploaded on the first use of a camera set; the context keeps
 *   them, keyed by the parameters' bytes.  OPK_ERR_ARG, before any device work: a destination that
 *   is not BGR, n not a multiple of V, a frame size other than its view's, every descriptor error
 *   and overlap rule of opk_frames / opk_frames_out (opk_render_frames_to); n == 0 succeeds
 *   without device work.  The cached maps are never evicted: every distinct camera set keeps its
 *   6 bytes per pixel and distinct camera (5.5 MB per camera at 1280x720) until opk_ctx_destroy --
 *   meant for a fixed rig, not for parameters that change from call to call. */
typedef struct opk_cameras {
    int views;                  /* V */
    const double* intrinsics;   /* [V][3][3] */
    const double* distortions;  /* [V][12]: the first ncoef[v] of a row are read */
    const int* ncoef;           /* [V]: 4, 5, 8 or 12 */
    const int* image_sizes;     /* [V][2]: width, height */
} opk_cameras;
int opk_undistort_maps_host(const opk_cameras* cams, int view, int16_t* m1_host, uint16_t* m2_host);
int opk_undistort_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* src,
                         const opk_cameras* cams);
/* The undistortion as the first stage of the raw-frame pipeline (--frame_undistort), under the
 * attach rules of opk_pose_attach_tracker: setting or clearing (cams NULL) with batches in flight
 * is OPK_ERR_STATE; the struct is copied.  While set, opk_pose_submit_frames first undistorts the
 * batch into a BGR buffer the batch's slot owns (it grows on demand; two slots, the two batches in
 * flight: 130 frames of 1280x720 are 360 MB per slot), and the frame warp, the tracker's pyramid,
 * the face / hand crops and the rig's size check read that buffer.  n not a multiple of V or a frame
 * size other than its view's is OPK_ERR_ARG at submit, before any device work.  Composes with
 * opk_pose_set_views (frame f is view f % V for both).
 * opk_pose_undistorted_frames: the description of the collected batch's buffer -- valid until the
 * second submit after that batch's, or until the cameras are cleared, which frees both slots'
 * buffers; hand it to the renders so the skeletons land on the undistorted image.  OPK_ERR_STATE
 * without cameras or without a batch collected with them. */
int opk_pose_set_undistort(opk_pose* pose, const opk_cameras* cams);
int opk_pose_undistorted_frames(opk_pose* pose, opk_frames* out);

/* ---- Rotated and flipped frames: op::rotateAndFlipFrame (utilities/openCv.cpp:236-282), which
 * the producer runs on every frame after the undistortion under --frame_rotate / --frame_flip
 * (producer.cpp:115-126) as a cv::transpose plus cv::flip on the host.
 *
 * ROTATED AND FLIPPED FRAMES.  The source S has h rows and w columns; rotate is in degrees, flip 0
 *   or 1.  r = rotate % 360 (C remainder) must be one of 0, +-90, +-180, +-270; anything else is
 *   OPK_ERR_ARG with the reference's words, "Rotation angle = R != {0, 90, 180, 270} degrees."
 *   (R = r).  -270, -180 and -90 mean 90, 180 and 270.  A flip other than 0 or 1 is OPK_ERR_ARG.
 *   The destination D is h x w for 0 and 180, and w rows x h columns for 90 and 270
 *   (opk_orient_size).  What rotateAndFlipFrame leaves:
 *
 *     rotate   flip 0: D[y][x] =      flip 1: D[y][x] =
 *        0     S[y][x]                S[y][w-1-x]
 *       90     S[x][w-1-y]            S[x][y]
 *      180     S[h-1-y][w-1-x]        S[h-1-y][x]
 *      270     S[h-1-x][y]            S[h-1-x][w-1-y]
 *
 *   (cv::transpose is T[y][x] = S[x][y]; cv::flip 0 mirrors the rows, 1 the columns, -1 both; the
 *   reference flips the transpose by 0 / none at 90 and by 1 / -1 at 270, the frame itself by
 *   none / 1 at 0 and by -1 / 0 at 180 -- flip 0 / flip 1 in each pair.  OpenCV is not needed to
 *   check the table: tests/orient_cases.py restates it as index arithmetic.)
 *
 * HOW EACH FORMAT MOVES.  The frames stay in their format; a sample is moved whole.  BGR moves
 *   pixels of 3 bytes.  NV12 and I420 move the Y plane by the table at (w, h) and the chroma by
 *   the same table at (w/2, h/2) -- NV12's (U, V) pair is one sample, I420's U and V are two
 *   planes.  Width and height are even, so 2x2 blocks go to 2x2 blocks: nothing is resampled.
 *   Hence opk_frames_to_bgr(orient(f)) equals orient(opk_frames_to_bgr(f)) bit for bit.  The same
 *   is NOT true of opk_bgr_to_frames, whose chroma comes from each block's top-left pixel, which a
 *   flip or a rotation moves to another corner.
 *
 * COORDINATES.  With the pipeline stage set, keypoints come out in the oriented frame's
 *   coordinates, as in the reference.  opk_orient_keypoints takes [people][parts][3] host arrays
 *   from source coordinates to oriented ones (inverse 0) or back (inverse 1), in place: the table
 *   applied to pixel indices -- for (90, 0), oriented (x, y) is source (w-1-y, x) -- each
 *   coordinate one fp32 subtraction from (float)(w-1) or (float)(h-1), or a copy; width and height
 *   are the source frame's.  A keypoint whose third value is 0 is left as it is (the reference's
 *   missing keypoint is (0, 0, 0)).  With inverse 1 a caller puts results back onto the original
 *   video.  A pure host function, as is opk_orient_size.
 *
 * opk_orient_frames: src -> dst, enqueued on the context's stream (kernels/orient.hip, one launch
 *   per plane).  OPK_ERR_ARG, before any device work: a destination of another format than the
 *   source, another n, a size other than opk_orient_size's, a source without area, and every
 *   descriptor error and overlap rule of opk_undistort_frames (in place is refused); n == 0
 *   succeeds without a launch.  Any row step, frame stride, odd BGR size and base alignment is
 *   taken: where every base, step and stride of both sides is a multiple of 4 the kernels move
 *   dwords, otherwise bytes. */
int opk_orient_size(int width, int height, int rotate, int* out_w, int* out_h);
int opk_orient_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* src, int rotate,
                      int flip);
int opk_orient_keypoints(float* keypoints_host, int people, int parts, int width, int height,
                         int rotate, int flip, int inverse);
/* The orientation as a stage of the raw-frame pipeline, under the attach rules of
 * opk_pose_set_undistort: setting or clearing with batches in flight is OPK_ERR_STATE; (0, 0)
 * clears the stage and frees both slots' buffers, and nothing is allocated or launched for it.
 * While set, opk_pose_submit_frames orients the batch -- after the undistortion when cameras are
 * set too (the reference's order), reading that stage's BGR buffer -- into a buffer the batch's
 * slot owns: the source's format, tight rows, grown on demand (one more buffer per slot).  The net
 * input size, the frame warp, the tracker's pyramid, the face / hand crops and the rig's size check
 * take the oriented frames and size; the cameras of opk_pose_set_undistort are checked against the
 * source size.  With a rig set (opk_pose_set_views) its image sizes must therefore be the oriented
 * ones -- at 90 degrees a rig of the source size is OPK_ERR_ARG at submit -- and supplying camera
 * matrices of the oriented images is the caller's job: nothing here rotates a camera matrix.
 * opk_pose_oriented_frames: the description of the collected batch's oriented buffer, under the
 * lifetime rule of opk_pose_undistorted_frames, for the renders; OPK_ERR_STATE without the stage or
 * without a batch collected with it.  opk_pose_undistorted_frames keeps returning the undistorted
 * buffer, which is not rotated. */
int opk_pose_set_orientation(opk_pose* pose, int rotate, int flip);
int opk_pose_oriented_frames(opk_pose* pose, opk_frames* out);
/* The calibration files: <dir>/<serial>.xml as the reference's writer emits them
 * (models/cameraParameters/flir/17012332.xml.example) -- an <opencv_storage> element whose children
 * CameraMatrix (3x4, the extrinsics), Intrinsics (3x3), Distortion (N x 1 or 1 x N, N in {4, 5, 8,
 * 12, 14}) and the optional CameraMatrixInitial (3x4) hold <rows>, <cols>, <dt> (d or f) and
 * whitespace-separated <data>; comments and the <?xml?> line are skipped.  Not a general XML
 * parser.  serials NULL: every *.xml of the directory, sorted by name (getFilesOnDirectory), n
 * ignored.  out [capacity] (NULL with capacity 0 to ask for *count alone); more cameras than
 * capacity is OPK_ERR_ARG.  camera_matrix is opk_camera_matrix(intrinsics, extrinsics).  A pure
 * host function.  OPK_ERR_ARG with the reference's wording -- "Error at reading the camera matrix
 * parameters of the camera with serial number `S` (file: P.xml). Is its format valid? You might
 * want to check the example xml file.", likewise "camera intrinsics parameters", "camera distortion
 * parameters" and, for a file that cannot be opened or holds no <opencv_storage>, "camera
 * parameters"; a missing CameraMatrixInitial is no error (has_initial 0, extrinsics_initial the
 * 3x4 identity).  A count that disagrees with rows x cols, or a number strtod does not consume
 * whole, is OPK_ERR_ARG with the file named. */
typedef struct opk_camera_parameters {
    char serial[256];
    double extrinsics[12];           /* CameraMatrix */
    double intrinsics[9];
    double distortion[14];           /* the first ncoef as read, zeros after */
    int ncoef;
    int has_initial;
    double extrinsics_initial[12];   /* CameraMatrixInitial */
    double camera_matrix[12];        /* intrinsics x extrinsics */
} opk_camera_parameters;
int opk_camera_parameters_read(const char* dir, const char* const* serials, int n,
                               opk_camera_parameters* out, int capacity, int* count);

/* ---- Measured ceilings (no reference counterpart; SURVEY.md §8d "confirm the vendor peaks"):
 *      dense fp16 MFMA rate of v_mfma_f32_16x16x32_f16 from registers (the conv kernels'
 *      instruction; 4 waves per SIMD, 8 independent chains, consecutive MFMAs on different operand
 *      pairs) on uniform random and on all-zero operands, in TFLOP/s, and the streaming HBM read
 *      rate over 2 GiB in GB/s.  Runs ~0.1 s of device work on the context's stream; synchronous. */
int opk_probe_peaks(opk_ctx* ctx, double* mfma_random_tflops, double* mfma_zero_tflops,
                    double* hbm_read_gbs);

/* ---- Renderers (enqueued on the context's stream).  frame_dev: the reference's float BGR frame
 *      [height][width][3] (0..255), drawn in place.
 * opk_render_pose_keypoints replaces op::renderPoseKeypointsGpu
 *   (include/openpose/pose/renderPose.hpp:14-18; src/openpose/pose/renderPose.cu:609-748 with
 *   renderKeypointsOld, include/openpose_private/utilities/render.hu:209-383): pose_dev
 *   [people][parts][3] (x, y, score) in frame pixels; every PoseModel, its pairs / colors / scales
 *   (pose/poseParametersRender.hpp), radius min(w,h)/100, line width min(w,h)/120; nothing is
 *   drawn for people == 0 unless blend_original == 0 (then the frame is cleared).  Errors as the
 *   reference: googly eyes with MPI, people > 127 (POSE_MAX_PEOPLE), an unknown model.  The
 *   reference's maxPtr / minPtr / scalePtr scratch is internal here.
 * opk_render_face_keypoints / opk_render_hand_keypoints replace op::renderFaceKeypointsGpu /
 *   op::renderHandKeypointsGpu (face/renderFace.hpp:12-15, hand/renderHand.hpp:12-15): 70 / 21
 *   parts, radius min/120 / min/100, line min/250 / min/80, no-op for count <= 0.
 * Keypoint renders take up to 1024 people (faces, hands) per call.
 * Heat-map renders (alpha outside [0, 1]: "Alpha must be in the range [0, 1]."; heat_dev
 *   [channels][heat_h][heat_w]; frame pixel x samples (x + 0.5) / scale_to_keep_ratio - 0.5):
 *   opk_render_pose_heat_map  = op::renderPoseHeatMapGpu  (renderPose.hpp:20-23): channel `part`,
 *                               bicubic, getColorHeatMap;
 *   opk_render_pose_heat_maps = op::renderPoseHeatMapsGpu (:25-28): every body part, nearest
 *                               sample, COCO colors;
 *   opk_render_pose_paf       = op::renderPosePAFGpu      (:30-33): PAF channels part, part + 1,
 *                               bilinear;
 *   opk_render_pose_pafs      = op::renderPosePAFsGpu     (:35-38): every PAF, from channel
 *                               parts + background;
 *   opk_render_pose_distance  = op::renderPoseDistanceGpu (:40-42): channel `part`, |bicubic|.
 * Arithmetic follows the reference expression by expression (each operation rounded); atan2f /
 * sinf / cosf are the HIP device library's (render parity unpinned at limb edges and for PAF
 * colours). */
int opk_render_pose_keypoints(opk_ctx* ctx, float* frame_dev, int pose_model, int people,
                              unsigned width, unsigned height, const float* pose_dev,
                              float render_threshold, int googly_eyes, int blend_original,
                              float alpha);
int opk_render_face_keypoints(opk_ctx* ctx, float* frame_dev, unsigned width, unsigned height,
                              const float* face_dev, int people, float render_threshold,
                              float alpha);
int opk_render_hand_keypoints(opk_ctx* ctx, float* frame_dev, unsigned width, unsigned height,
                              const float* hands_dev, int hands, float render_threshold,
                              float alpha);
int opk_render_pose_heat_map(opk_ctx* ctx, float* frame_dev, unsigned width, unsigned height,
                             const float* heat_dev, int heat_w, int heat_h,
                             float scale_to_keep_ratio, unsigned part, float alpha);
int opk_render_pose_heat_maps(opk_ctx* ctx, float* frame_dev, int pose_model, unsigned width,
                              unsigned height, const float* heat_dev, int heat_w, int heat_h,
                              float scale_to_keep_ratio, float alpha);
int opk_render_pose_paf(opk_ctx* ctx, float* frame_dev, int pose_model, unsigned width,
                        unsigned height, const float* heat_dev, int heat_w, int heat_h,
                        float scale_to_keep_ratio, int part, float alpha);
int opk_render_pose_pafs(opk_ctx* ctx, float* frame_dev, int pose_model, unsigned width,
                         unsigned height, const float* heat_dev, int heat_w, int heat_h,
                         float scale_to_keep_ratio, float alpha);
int opk_render_pose_distance(opk_ctx* ctx, float* frame_dev, unsigned width, unsigned height,
                             const float* heat_dev, int heat_w, int heat_h,
                             float scale_to_keep_ratio, unsigned part, float alpha);

/* ---- The output image: the two stages around the renderers, and all three in one pass for a
 *      batch of frames (enqueued on the context's stream).
 * opk_cvmat_to_output replaces op::CvMatToOpOutput::createArray, CPU branch
 *   (src/openpose/core/cvMatToOpOutput.cpp:76-149), for a batch: frames_dev = n BGR uint8 frames
 *   [height][step bytes] (step 0 = width*3) -> output_dev float [n][out_h][out_w][3].
 *   resizeFixedAspectRatio (openCvPrivate.cpp:34-53): cv::warpAffine(diag(scale)) with OpenCV's
 *   fixed-point 8-bit arithmetic, INTER_CUBIC for scale > 1 else INTER_LINEAR, zero border; the
 *   plain copy when scale == 1 and the sizes match.  Errors as the reference: "Output resolution
 *   has 0 area.", "Input images has 0 area.".
 * opk_output_to_cvmat replaces op::OpOutputToCvMat::formatToCvMat
 *   (src/openpose/core/opOutputToCvMat.cpp:77-130) for a batch: float [n][h][w][3] -> uint8
 *   [n][h][dst_step] (dst_step 0 = w*3; bytes of a row beyond w*3 are not written), with the cast
 *   of its CPU branch or of its GPU branch. */
#define OPK_CAST_CPU 0  /* cv::Mat::convertTo(CV_8UC3): saturate_cast<uchar>(cvRound(v)) -- round
                           to nearest, ties to even, then clamp to [0, 255]                     */
#define OPK_CAST_CUDA 1 /* uCharImageCast (gpu/cuda.cu:27-34): (uchar) fastTruncateCuda(v, 0,
                           255) -- clamp, then truncate toward zero                             */
int opk_cvmat_to_output(opk_ctx* ctx, float* output_dev, const uint8_t* frames_dev, int n,
                        int width, int height, size_t step, double scale, int out_w, int out_h);
int opk_cvmat_to_output_fmt(opk_ctx* ctx, float* output_dev, const opk_frames* frames, double scale,
                            int out_w, int out_h);
int opk_output_to_cvmat(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, const float* output_dev,
                        int n, int w, int h, int cast);

/* One keypoint layer of opk_render_frames: what one of opk_render_pose_keypoints / _face_ /
 * _hand_ would draw on each frame. */
#define OPK_LAYER_POSE 0
#define OPK_LAYER_FACE 1
#define OPK_LAYER_HAND 2
typedef struct opk_render_layer {
    int kind;                   /* OPK_LAYER_*                                                 */
    int pose_model;             /* POSE only                                                   */
    const float* keypoints_dev; /* [sum(counts)][parts][3], frame 0's first, in output pixels  */
    const int* counts_host;     /* [n]: people (faces, hands) of each frame                    */
    float render_threshold, alpha;
    int googly_eyes;            /* POSE only                                                   */
} opk_render_layer;

/* opk_render_frames: CvMatToOpOutput -> the layers in order -> OpOutputToCvMat for n frames in
 *   one pass per pixel; the float image is never written to memory.  dst_dev uint8
 *   [n][out_h][dst_step] (dst_step 0 = out_w*3).  blend_original == 0 clears each frame before the
 *   first layer (renderPoseKeypointsGpu's blendOriginalFrame).  0..3 layers; with 0 layers this is
 *   the warp + cast alone.  Per frame at most 127 people in a POSE layer (the reference's
 *   POSE_MAX_PEOPLE error) and 1024 in a FACE / HAND layer.  The result bytes are exactly those of
 *   opk_cvmat_to_output -> opk_render_*_keypoints per frame and layer -> opk_output_to_cvmat.
 *   Argument errors (the renderers' texts) are raised before any device work; n == 0 succeeds
 *   with none.
 * opk_pose_render_frames: the last collected batch of a pose pipeline drawn on its frames: uploads
 *   the batch's keypoints (x, y times scale_input_to_output) as one POSE layer of the pipeline's
 *   model and calls opk_render_frames.  OPK_ERR_STATE when nothing is collected or n is not the
 *   collected batch's frame count. */
int opk_render_frames(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                      const uint8_t* frames_dev, int n, int width, int height, size_t step,
                      double scale_input_to_output, const opk_render_layer* layers, int n_layers,
                      int blend_original, int cast);
int opk_pose_render_frames(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                           const uint8_t* frames_dev, int n, int width, int height, size_t step,
                           double scale_input_to_output, float render_threshold, float alpha,
                           int googly_eyes, int blend_original, int cast);
/* The same on opk_frames descriptors (see opk_frames); the drawn images stay BGR uint8 (NV12 /
 * I420 out: opk_render_frames_to, opk_pose_render_frames_to below). */
int opk_render_frames_fmt(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                          const opk_frames* frames, double scale_input_to_output,
                          const opk_render_layer* layers, int n_layers, int blend_original,
                          int cast);
int opk_pose_render_frames_fmt(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w,
                               int out_h, const opk_frames* frames, double scale_input_to_output,
                               float render_threshold, float alpha, int googly_eyes,
                               int blend_original, int cast);
/* opk_pose_render_frames with the face / hand stages' results (opk_pose_attach_extractor): the
 * collected batch as one POSE layer, then one FACE layer and one HAND layer, each only if its
 * extractor is attached, through opk_render_frames -- the bytes are opk_render_frames' for those
 * layers.  A frame's HAND layer holds the left hands of its people in person order, then the right
 * hands (opk_pose_part_keypoints' layout), its FACE layer one face per person; x and y of every
 * layer are multiplied by scale_input_to_output in float. */
int opk_pose_render_frames_parts(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w,
                                 int out_h, const uint8_t* frames_dev, int n, int width, int height,
                                 size_t step, double scale_input_to_output, float render_threshold,
                                 float alpha, int googly_eyes, int blend_original, int cast,
                                 float face_threshold, float face_alpha, float hand_threshold,
                                 float hand_alpha);
int opk_pose_render_frames_parts_fmt(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w,
                                     int out_h, const opk_frames* frames,
                                     double scale_input_to_output, float render_threshold,
                                     float alpha, int googly_eyes, int blend_original, int cast,
                                     float face_threshold, float face_alpha, float hand_threshold,
                                     float hand_alpha);

/* The heat layer of opk_render_frames_heat: what one of opk_render_pose_heat_map / _heat_maps /
 * _paf / _pafs / _distance would draw on each frame, from frame f's own stack of heat_dev. */
#define OPK_HEAT_NONE 0     /* opk_render_element only: element 0, the keypoints               */
#define OPK_HEAT_PART 1     /* opk_render_pose_heat_map, channel `channel`                     */
#define OPK_HEAT_PARTS 2    /* opk_render_pose_heat_maps of pose_model                         */
#define OPK_HEAT_PAF 3      /* opk_render_pose_paf, channels `channel`, `channel` + 1          */
#define OPK_HEAT_PAFS 4     /* opk_render_pose_pafs of pose_model                              */
#define OPK_HEAT_DISTANCE 5 /* opk_render_pose_distance, channel `channel`                     */
typedef struct opk_render_heat {
    int kind;               /* OPK_HEAT_PART, OPK_HEAT_PARTS, OPK_HEAT_PAF, OPK_HEAT_PAFS, OPK_HEAT_DISTANCE */
    int pose_model;
    int channel;            /* PART / DISTANCE: the channel; PAF: its first channel */
    const float* heat_dev;  /* [n][channels][heat_h][heat_w] */
    int channels, heat_w, heat_h;
    float scale_to_keep_ratio, alpha;
} opk_render_heat;

/* opk_render_frames_heat: opk_render_frames with a heat layer drawn after the warp and before the
 *   0..3 keypoint layers -- every element op::PoseGpuRenderer::renderPose can draw
 *   (src/openpose/pose/poseGpuRenderer.cpp:102-202, --part_to_show) for a batch, in the same one
 *   pass per pixel.  The result bytes are exactly those of opk_cvmat_to_output -> the matching
 *   opk_render_pose_* heat call per frame -> opk_render_*_keypoints per frame and layer (blending
 *   on) -> opk_output_to_cvmat.  A tile's heat samples are evaluated once into LDS where their
 *   window fits it and per pixel where it does not; the bytes are the same.
 *   Errors before any device work, OPK_ERR_ARG: "Alpha must be in the range [0, 1].", "Invalid
 *   Model." (PARTS, PAF, PAFS), an unknown kind, a channel outside the stack, an empty heat map,
 *   heat_dev NULL with n > 0, and blend_original == 0 (the heat renders never clear the frame: the
 *   reference expresses "no blending" as alpha 1).  heat NULL: opk_render_frames.
 * opk_render_element: host-only; the heat kind and channel of renderPose's elementRendered for a
 *   model of P parts, background flag b, PB = P + b and N pairs: 0 the keypoints (OPK_HEAT_NONE);
 *   1 channel P if b else 0; 2 all parts; 3 all PAFs; 4 .. PB+2 part e - 3 - b; PB+3 .. PB+2+N the
 *   PAF whose first channel is PB + map_idx[2 (e - PB - 3)]; above that, for BODY_25D only (else
 *   "Neck-part distance channel only for BODY_25D."), its 2 (P - 1) distance channels
 *   PB + 2N + (e - (PB+2+N) - 1).  An element below 0 or past the model's last
 *   (getNumberElementsToRender, poseParametersRender.cpp:98-113) is OPK_ERR_ARG.
 * opk_pose_render_frames_element: element 0 is opk_pose_render_frames (alpha_keypoint); any other
 *   element of the pipeline's model is drawn as the heat layer, without keypoints, straight from
 *   the collected batch's net output (the lazy resize/merge of the pipeline, CPU or CUDA map
 *   semantics, 1..N scales): the full-resolution stack is neither written nor read.  Scale
 *   scale_net_to_output * scale_input_to_output, alpha blend_original ? alpha_heatmap : 1, as
 *   renderPose.  OPK_ERR_STATE when nothing is collected, n is not the batch's frame count, or a
 *   later batch is in flight (its net forward overwrites the net output). */
int opk_render_frames_heat(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w, int out_h,
                           const uint8_t* frames_dev, int n, int width, int height, size_t step,
                           double scale_input_to_output, const opk_render_layer* layers,
                           int n_layers, int blend_original, int cast,
                           const opk_render_heat* heat);
int opk_render_element(int pose_model, int element, int* kind, int* channel);
int opk_pose_render_frames_element(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w,
                                   int out_h, const uint8_t* frames_dev, int n, int width,
                                   int height, size_t step, double scale_input_to_output,
                                   int element, float render_threshold, float alpha_keypoint,
                                   float alpha_heatmap, int googly_eyes, int blend_original,
                                   int cast);
/* Both on opk_frames descriptors (see opk_frames). */
int opk_render_frames_heat_fmt(opk_ctx* ctx, uint8_t* dst_dev, size_t dst_step, int out_w,
                               int out_h, const opk_frames* frames, double scale_input_to_output,
                               const opk_render_layer* layers, int n_layers, int blend_original,
                               int cast, const opk_render_heat* heat);
int opk_pose_render_frames_element_fmt(opk_pose* pose, uint8_t* dst_dev, size_t dst_step, int out_w,
                                       int out_h, const opk_frames* frames,
                                       double scale_input_to_output, int element,
                                       float render_threshold, float alpha_keypoint,
                                       float alpha_heatmap, int googly_eyes, int blend_original,
                                       int cast);

/* The drawn frames into an opk_frames_out destination -- BGR, NV12 or I420 (see opk_frames_out:
 * out_w, out_h are dst->width, dst->height; the YUV samples are opk_bgr_to_frames of the BGR
 * call's bytes, converted in the render's store epilogue).  Every argument and state error of the
 * call being wrapped keeps its code and text.
 * opk_render_frames_to: opk_render_frames_heat_fmt (heat NULL: opk_render_frames_fmt).
 * opk_pose_render_frames_to: opk_pose_render_frames_element_fmt; with part_params = {face_threshold,
 *   face_alpha, hand_threshold, hand_alpha} opk_pose_render_frames_parts_fmt with alpha_keypoint as
 *   its alpha (element must then be 0). */
int opk_render_frames_to(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* frames,
                         double scale_input_to_output, const opk_render_layer* layers, int n_layers,
                         int blend_original, int cast, const opk_render_heat* heat);
int opk_pose_render_frames_to(opk_pose* pose, const opk_frames_out* dst, const opk_frames* frames,
                              double scale_input_to_output, int element, float render_threshold,
                              float alpha_keypoint, float alpha_heatmap, int googly_eyes,
                              int blend_original, int cast, const float* part_params);

/* ---- Frames to JPEG files: what op::ImageSaver leaves under --write_images_format jpg and, frame
 * by frame, under --write_video (saveImage -> cv::imwrite with the default parameters of
 * filestream/fileStream.hpp:54-57, quality 100; videoSaver.cpp:110-121).  cv::imwrite drives
 * libjpeg(-turbo) with its defaults: JFIF, YCbCr 4:2:0, JDCT_ISLOW, the standard Huffman tables,
 * force_baseline.  The bar is equality of files with that library, not PSNR.
 *
 * JPEG FRAMES.  One file per frame of w x h pixels (each in 1..65535) at quality q in 1..100.
 *
 *   FILE LAYOUT (multi-byte fields big-endian): FFD8; APP0 of length 16 -- "JFIF\0", version 1.01,
 *   units 0, density 1 x 1, no thumbnail; DQT id 0 (luma) and DQT id 1 (chroma), 64 bytes each in
 *   zigzag order, 8-bit; SOF0 -- precision 8, height, width, 3 components (1, 0x22, 0), (2, 0x11, 1),
 *   (3, 0x11, 1); DHT class 0 id 0, class 1 id 0, class 0 id 1, class 1 id 1 (T.81 Annex K.3, K.5,
 *   K.4, K.6); SOS -- 3 components (1, 0x00), (2, 0x11), (3, 0x11), then 0, 63, 0; the
 *   entropy-coded data; FFD9.  No restart markers, no comments.  The header is 623 bytes for every
 *   size and quality.  The tables are constants (kernels/jpeg_tables.inc).
 *
 *   QUALITY (jpeg_quality_scaling): s = 5000 / q for q < 50, else 200 - 2q; Q[k] = clamp((base[k] * s
 *   + 50) / 100, 1, 255) with base the Annex K.1 (luma) and K.2 (chroma) tables.  q = 100 gives all
 *   ones: the reference's default.
 *
 *   COLOUR, int32 with an arithmetic >>, on the R, G, B of a BGR pixel:
 *     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *
 *   EDGES.  The full-resolution planes are padded by replication to the width 16 * ceil(w / 16) and
 *   to an even height.  Chroma is then downsampled 2 x 2 as (a + b + c + d + bias) >> 2, bias 1 in
 *   even output columns and 2 in odd ones, and after that its last real row, row ceil(h / 2) - 1,
 *   is replicated downwards; the last luma row is replicated downwards.  (So below an even height
 *   that is no multiple of 16 the chroma repeats the mean of the last two rows, the luma the last
 *   row alone.)
 *
 *   BLOCKS.  A component has ceil(w_c / 8) x ceil(h_c / 8) real blocks.  An MCU is Y(0,0), Y(0,1),
 *   Y(1,0), Y(1,1), Cb, Cr (row, column), MCUs row by row.  A luma block of an MCU outside the real
 *   blocks (a dummy block) is not transformed: its ACs are 0 and its DC is the quantised DC of the
 *   block before it in that MCU.  An MCU's chroma blocks are always real.
 *
 *   FDCT (jfdctint.c, CONST_BITS 13, PASS1_BITS 2) on samples - 128, rows first, then columns, with
 *   DESCALE(x, n) = (x + (1 << (n - 1))) >> n and FIX(c) = round(c * 8192).  One pass over d0..d7:
 *     t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5,
 *     t3 = d3 + d4, t4 = d3 - d4;  t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *     rows:    o0 = (t10 + t11) << 2,        o4 = (t10 - t11) << 2,        n = 11
 *     columns: o0 = DESCALE(t10 + t11, 2),   o4 = DESCALE(t10 - t11, 2),   n = 15
 *     z1 = (t12 + t13) FIX(0.541196100)
 *     o2 = DESCALE(z1 + t13 FIX(0.765366865), n),  o6 = DESCALE(z1 - t12 FIX(1.847759065), n)
 *     z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) FIX(1.175875602)
 *     t4 *= FIX(0.298631336), t5 *= FIX(2.053119869), t6 *= FIX(3.072711026), t7 *= FIX(1.501321110)
 *     z1 *= -FIX(0.899976223), z2 *= -FIX(2.562915447),
 *     z3 = -z3 FIX(1.961570560) + z5, z4 = -z4 FIX(0.390180644) + z5
 *     o7 = DESCALE(t4 + z1 + z3, n), o5 = DESCALE(t5 + z2 + z4, n),
 *     o3 = DESCALE(t6 + z2 + z3, n), o1 = DESCALE(t7 + z1 + z4, n)
 *   Every intermediate fits int32.
 *
 *   QUANTISATION.  With qv = 8 Q in natural order, c = sign(f) * ((|f| + (qv >> 1)) / qv); the block
 *   is then read in zigzag order.
 *
 *   ENTROPY CODING.  The DC difference is taken against the previous block of the same component
 *   in stream order, dummy blocks included, from 0 at the start of a frame.  A value v has size
 *   n = bit_length(|v|); its n extra bits are v for v >= 0, else the low n bits of v - 1.  An AC is
 *   coded as the symbol (run << 4 | n), after one ZRL (0xF0) for each full run of 16 zeros before
 *   it; EOB (0x00) follows when the block ends in zeros.  Bits go MSB first, the last byte is
 *   filled with 1-bits, and a 0x00 follows every 0xFF data byte, a last byte made 0xFF by the fill
 *   included.
 *
 *   OTHER FORMATS.  An NV12 or I420 source gives the file of opk_frames_to_bgr(frames): JFIF is
 *   full range and these formats are limited range, so nothing is taken from the planes directly.
 *
 * opk_jpeg_bound: a capacity that n frames of w x h can never exceed (derived in host/jpeg.cpp:
 *   1660 bits per block at most, doubled by stuffing, plus 625 bytes); 0 for nothing to encode.
 * opk_jpeg_encode_host: the plain C++ encoder of n host BGR frames (step, frame_bytes: 0 = tight);
 *   needs no context and no device.
 * opk_jpeg_encode: the same files from device frames, enqueued on the context's stream
 *   (kernels/jpeg.hip).  Frame f's file is dst[offsets[f] .. offsets[f + 1]): the files are packed,
 *   offsets[0] = 0, offsets has n + 1 entries.  A frame whose end would pass `capacity` is not
 *   written at all, nor is any frame after it; the offsets are still the true ones, so
 *   offsets[n] > capacity tells how much room the batch needs.  No byte at or past dst + capacity
 *   is touched.  The files do not depend on the order in which workgroups arrive: they are the same
 *   from run to run and the same as the host route's.
 * OPK_ERR_ARG, before any work: every descriptor error of opk_frames, a width or height outside
 *   1..65535, a quality outside 1..100, a NULL dst or offsets with n > 0, dst overlapping the
 *   source.  n == 0 succeeds: offsets[0] = 0 on the host route, no launch on the device route. */
size_t opk_jpeg_bound(int n, int w, int h);
int opk_jpeg_encode_host(uint8_t* dst, size_t capacity, uint64_t* offsets, const uint8_t* bgr,
                         size_t step, size_t frame_bytes, int n, int w, int h, int quality);
int opk_jpeg_encode(opk_ctx* ctx, uint8_t* dst_dev, size_t capacity, uint64_t* offsets_dev,
                    const opk_frames* frames, int quality);

#ifdef __cplusplus
}
#endif
#endif /* OPK_H */
