// net.h -- NetHip: the op::NetCaffe replacement (graph planner + gfx950 executor).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/conv.h"
#include "context.h"
#include "graph.h"

namespace opk {

class NetHip {
public:
    NetHip(Context* ctx, std::vector<LayerDesc> layers, const std::string& output_blob = "net_output");

    struct ConvInfo {
        std::string name;
        int cin, cout, k, act;   // act: 0 none, 1 ReLU, 2 PReLU
        std::string act_layer;   // the fused ReLU/PReLU layer (holds the PReLU slopes)
    };
    const std::vector<ConvInfo>& convs() const { return info_; }
    void set_conv(const std::string& name, const float* w, const float* b, const float* slope);
    // Arithmetic of the forward: kPrecisionFp16 (default: fp16 weights and stored activations,
    // fp32 MFMA accumulation, the tuned fused kernels) or kPrecisionSplit (every weight and
    // activation as an fp16 hi / lo pair, three MFMA passes per conv on conv3_kernel, no fused
    // kernels: ~fp32 results at ~3x the MFMA work; ConvArgs::split).  Re-plans the shapes and
    // re-packs the loaded weights.
    static constexpr int kPrecisionFp16 = 0, kPrecisionSplit = 1;
    void set_precision(int precision);   // the uniform schedule
    // Per-layer precision: one kPrecisionFp16 / kPrecisionSplit per conv, in convs() order.  An
    // fp16 conv reads the hi image of its source and writes hi only (the lo twin of its channels,
    // where the buffer has one, keeps the zero the plan's memset gave it); a split conv reads hi
    // and lo and writes both.  Planning rules (dispatch()):
    //   * a buffer has a lo twin iff a split conv (or a pool fed by one) writes some of its
    //     channels, or a three-product kernel has to read it (below);
    //   * a split conv none of whose input channels has a split writer is "hi-only": it runs the
    //     two-product instantiation (Conv3Plan::xhi) where its tile has one, else the
    //     three-product kernel over a zero twin the plan allocates for it;
    //   * conv1 fusion needs both convs fp16; a head pair runs fused only with equal precisions;
    //     a pool follows its input (split iff the input has a twin).
    // Refuses (OPK_ERR_ARG, the schedule in force untouched) a wrong count or an unknown value.
    // Re-packs only the convs whose precision changes and re-plans the shapes.
    void set_precision_schedule(const int* precisions, int count);
    int conv_precision(int index) const;   // -1: bad index
    // Small-batch mode (off by default): 3x3 convs whose product geometry gives fewer
    // workgroups than the chip has CUs run on conv3s tiles (conv3_plan, conv.h) -- the same
    // bits, more of the chip busy when a forward is a frame or a few.  Re-plans the shapes.
    void set_small_batch(bool on);
    bool small_batch() const { return small_batch_; }
    // host-only: the GEMM tile, fill measure (Conv3Plan::workgroups) and kernel family (small:
    // conv3s) the planner picks for conv `index` of an n x h x w forward on a chip of cus compute
    // units (the image conv: zeros)
    void conv_plan(int index, int n, int h, int w, int cus, int* bm, int* bn, int* workgroups,
                   int* small) const;
    // host-only: the launch-log name prefix (Conv3Plan::name) of every launch such a forward
    // makes for conv `index`, in launch order: one per frame run; a conv inside conv1_fused_kernel
    // or conv_head_kernel gives that kernel's name on the unit's first conv and nothing on the
    // others; the image conv gives conv_image_kernel
    std::vector<std::string> conv_kernels(int index, int n, int h, int w, int cus) const;
    bool ready() const;
    // caffe::Net::CopyTrainedLayersFrom (netCaffe.cpp:165,185): weights, bias and PReLU slopes of
    // every conv named in the file (shapes checked as Caffe does); layers the net does not have
    // are ignored.  Returns the number of convolutions loaded.
    int load_caffemodel(const std::string& path);

    // input: device NCHW fp32 [n][3][h][w].  Every input shape gets its own plan (activation
    // buffers with zeroed guards, launch arguments, net output), kept across forwards, so the
    // scales of a multi-scale pass alternate without re-planning and their outputs coexist.
    void forward(const float* input, int n, int h, int w);
    // the same on another stream, optionally untimed (concurrent scales, PoseHip::submit_multi);
    // prepare() plans a shape ahead (its buffers are zeroed on the context stream)
    void forward_on(const float* input, int n, int h, int w, hipStream_t stream, bool timed);
    void prepare(int n, int h, int w);
    void time_begin(hipStream_t s) { timer_.begin(s); }
    void time_end(hipStream_t s) { timer_.end(s); }
    // net output of the last forward ([n][out_channels][out_h][out_w] fp32, stays valid until
    // set_conv or until more than kMaxShapes other shapes have been planned; a shape forwarded by
    // the pose pipeline alternates between two output buffers, select_output)
    float* output() const { return cur_ ? cur_->out() : nullptr; }
    // plans the shape and returns the output buffer its next forward writes; alternate: switch to
    // the shape's other buffer first (PoseHip: batch i+1's nets need not wait for the
    // post-processing of batch i, which reads the first)
    float* select_output(int n, int h, int w, bool alternate);
    // Readers of an output buffer outside the forward's stream order (PoseHip's post-processing
    // stream): ev was recorded after the last such read of out.  Every later forward that writes
    // out -- through PoseHip or a direct opk_net_forward -- first makes its stream wait for ev, so
    // the forward never overwrites values a post-processing still reads.  One event per buffer
    // (the readers run in order on one stream, so the latest covers the earlier ones).
    // expires when the net is destroyed: a PoseHip holding this net detects a net destroyed
    // before it (~PoseHip's forget_reader_events on a dead net)
    std::weak_ptr<void> liveness() const { return alive_; }
    void note_reader(const float* out, hipEvent_t ev);
    void forget_reader_events(const hipEvent_t* evs, int n);   // (the owner destroys them)
    int out_channels() const { return out_c_; }
    int out_h() const { return cur_ ? cur_->lh[out_level_] : 0; }
    int out_w() const { return cur_ ? cur_->lw[out_level_] : 0; }
    int frames() const { return cur_ ? cur_->n : 0; }
    static constexpr int kMaxShapes = 8;
    double flops_per_frame(int h, int w) const;   // useful (unpadded) conv FLOPs
    int border() const { return border_; }
    ~NetHip();

    // forward timing on the context stream (HIP events around every forward while enabled);
    // read() waits for the recorded forwards and returns their count and summed milliseconds
    void set_timing(bool on);
    void read_timing(int* count, double* total_ms);

    // caffe::Net::blob_by_name for the last forward (inspection / per-layer tests): frames
    // [f0, f0 + nf) of a named conv / pool / concat top as fp32 NCHW host [nf][ch][h][w], read from
    // its padded NHWC fp16 buffer (or the fp32 net output).  Blobs the fused kernels keep on chip
    // (conv1_1 / conv1_2 in conv1_fused, a pooled conv's un-pooled output, Mconv6 in conv_head)
    // throw.  host == nullptr: shape only.
    void blob(const std::string& name, int f0, int nf, float* host, int shape[4]) const;
    // the same, the stored planes apart: the hi image and its lo twin (zeros and *has_lo = 0 where
    // the buffer has none; the fp32 net output: hi = the value).  Either plane may be nullptr.
    void blob_planes(const std::string& name, int f0, int nf, float* hi, float* lo, int shape[4],
                     int* has_lo) const;
    // kernels launched by the last forward run while the dev switch LAUNCH_LOG was 1
    const std::vector<std::string>& launches() const { return log_.lines; }

private:
    struct Placement { int buf; int coff; };
    struct BufSpec { int level; int cs; };
    struct ConvPlan {
        ConvInfo info;
        std::string in_blob;
        int level = 0;
        bool from_image = false;
        Placement in{};
        int cin_pad = 0, ntaps = 9, ksteps = 0, bn = 128, cout_pad = 0;
        std::vector<Placement> outs;
        int out32_coff = -1;
        DevBuf w, bias, slope;
        DevBuf w3;            // halo-kernel weight layout (3x3 convs)
        DevBuf wh;            // conv_head.hip layout when this conv is half of a fused head pair
        int head = -1;        // index into heads_ (as either half), -1 none
        bool loaded = false;
        bool slope01 = true;  // PReLU slopes all in [0, 1] (ConvArgs::actmax)
        float wscale = 1.f;   // split precision: 2^-e of the packed weights' scaling (ConvArgs::wscale)
        int precision = kPrecisionFp16;   // this conv's arithmetic (set_precision_schedule)
        std::vector<float> hw, hb, hs;   // host copies of the weights (re-packed per precision)
    };
    bool fused1_at(int h, int w) const;            // conv1_fused_kernel runs at this input size
    void read_planes(const std::string& name, int f0, int nf, float* hi, float* lo, float* sum,
                     int shape[4], int* has_lo) const;
    void pack(ConvPlan& c);   // device layouts of one conv's weights for its precision
    struct PoolPlan { int in_buf, out_buf, level_in, channels; };
    struct Step { bool conv; int idx; };

    // what runs for one input shape on a chip of cus compute units: decided on the host, before
    // any device memory exists (dispatch())
    struct Dispatch {
        std::vector<int> lh, lw;       // size of every pooling level
        std::vector<char> csplit;      // per conv: kPrecisionSplit
        std::vector<char> twin;        // per buffer: has a lo twin
        bool fused1 = false;           // conv1_fused_kernel runs for this shape
        std::vector<char> headfused;   // per head pair: conv_head_kernel runs it
        std::vector<char> poolfused;   // per pool: run inside its conv's epilogue (conv3w8 POOL)
        std::vector<Conv3Query> query; // per conv (not the image conv): the whole batch's query
        std::vector<Conv3Plan> conv;   // ... and its plan
        // per conv that runs a halo kernel of its own (not the image conv, not inside
        // conv1_fused_kernel / conv_head_kernel): its launches (conv3_runs)
        std::vector<std::vector<Conv3Run>> runs;
    };
    Dispatch dispatch(int n, int h, int w, int cus) const;
    std::vector<int> level_sizes(int size) const;   // a side of every pooling level

    struct PoolArgs {
        uint16_t *out, *out_lo;        // (lo twins: the split pool)
        const uint16_t *in, *in_lo;
        int frames, H, W, C, OH, OW;
    };
    // One kernel launch of a forward, its arguments finished when the shape is planned
    // (launch_list()); a forward replays the list and fills in only the input pointer and the
    // fp32 output buffer it writes (ShapePlan::out()).
    struct Launch {
        enum Kind { kConv1Fused, kConvHead, kConvImage, kConv3, kPool } kind;
        std::string layer;             // launch-log label
        Conv1FusedArgs fused1{};       // kConv1Fused
        HeadArgs head{};               // kConvHead
        ConvArgs conv{};               // kConvImage; kConv3: pointers at the run's first frame
        Conv3Plan plan{};              // kConv3: the run's plan
        PoolArgs pool{};               // kPool
        long out32 = -1;               // kConvHead / kConv3 writing the net output: the floats
                                       // between the output buffer's start and the run's first frame
    };

    // shape-dependent state of one input shape
    struct ShapePlan : Dispatch {
        int n = 0, h = 0, w = 0;
        int cus = 0;                   // compute units planned for (GRID_CUS)
        std::vector<std::unique_ptr<DevBuf>> mem;
        std::vector<uint16_t*> base;   // first position of each buffer (past its head guard)
        std::vector<std::unique_ptr<DevBuf>> mem_lo;
        std::vector<uint16_t*> base_lo;
        DevBuf out_mem, out_mem_alt;
        float* out32 = nullptr;
        float* out32_alt = nullptr;    // the second output buffer (select_output)
        bool alt = false;              // forwards write out32_alt
        float* out() const { return alt ? out32_alt : out32; }
        std::vector<Launch> launches;  // a forward, in launch order
    };

    void plan(const std::vector<LayerDesc>& layers);
    std::vector<Launch> launch_list(const ShapePlan& S, void* sink) const;
    void forward_launches(ShapePlan& S, const float* input, hipStream_t st);
    void forward_steps(ShapePlan& S, const float* input, hipStream_t st);
    ShapePlan* shape_plan(int n, int h, int w, hipStream_t zero_stream = nullptr);

    Context* ctx_;
    std::string output_blob_;
    std::vector<ConvInfo> info_;
    std::vector<ConvPlan> convs_;
    std::map<std::string, int> conv_by_name_;
    std::vector<PoolPlan> pools_;
    std::vector<Step> steps_;
    std::vector<BufSpec> bufs_;
    int out_level_ = 0, out_c_ = 0, nlevels_ = 1;
    int image_buf_ = -1;
    struct Fuse1 { int a = -1, b = -1, p = -1, abuf = -1, bbuf = -1; };
    Fuse1 fuse1_;                 // conv1_1 -> conv1_2 -> pool1 (conv1_fused.hip) when planned
    // Mconv6 -> Mconv7 pairs (conv_head.hip): a = 1x1 conv with 256 / 512 outputs read only by b,
    // a 1x1 conv with <= 64 outputs, consecutive steps; buf = a's output buffer
    struct FuseHead { int a = -1, b = -1, step = -1, buf = -1; };
    std::vector<FuseHead> heads_;
    // conv -> 2x2 max pool pairs (conv3w8.hip POOL epilogue), per pool: the conv that alone feeds it
    // (and nothing else reads), -1 none; per input shape it runs fused where conv3w8 supports it
    std::vector<int> pool_conv_;
    int cus_ = 256;               // compute units (persistent-kernel grid)
    bool small_batch_ = false;    // set_small_batch
    int border_ = 1;              // zero border of every padded image (widest conv pad, >= 1)

    struct BlobLoc { int buf = -1, coff = 0, ch = 0, level = 0; bool out32 = false; };
    std::map<std::string, BlobLoc> blob_loc_;   // every named top (plan)
    LaunchLog log_;

    std::vector<std::unique_ptr<ShapePlan>> shapes_;   // oldest first
    ShapePlan* cur_ = nullptr;    // shape of the last forward
    std::vector<std::pair<const float*, hipEvent_t>> readers_;   // note_reader
    std::shared_ptr<int> alive_ = std::make_shared<int>(0);       // liveness()
    DevBuf sink_;                 // persistent conv3: target of masked-off stores
    EventTimer timer_;            // forwards bracketed by HIP events (set_timing)
};

}  // namespace opk
