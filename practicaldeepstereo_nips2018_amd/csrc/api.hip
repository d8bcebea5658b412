// C ABI of libpds_hip.so (include/pds_hip.h): argument checks, workspace carving and the
// per-module launch sequences.  No allocation, no synchronisation: everything is enqueued on the
// caller's stream into caller-owned memory.
#include <cmath>

#include "api_internal.hpp"

namespace pds {

static thread_local char g_error[512] = "";

int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error((int)e, "%s: %s", what, hipGetErrorString(e));
    // PDS_DEBUG_SYNC=1 (debugging only): wait for every launch and name it, so that a faulting kernel is the
    // last line printed.  Off by default: the library never synchronises.
    static const bool debug_sync = getenv("PDS_DEBUG_SYNC") != nullptr;
    if (debug_sync) {
        fprintf(stderr, "[pds] %s ...", what);
        fflush(stderr);
        const hipError_t es = hipDeviceSynchronize();
        fprintf(stderr, " %s\n", es == hipSuccess ? "ok" : hipGetErrorString(es));
        if (es != hipSuccess) return set_error((int)es, "%s: %s", what, hipGetErrorString(es));
    }
    return 0;
}

// ---- launch probe (include/pds_hip.h, ABI v5): in-situ kernel timing for bench.py --------------------------------
namespace {
constexpr int kProbeMax = 256;
std::atomic<int> g_probe_armed{0};
char g_probe_name[64] = "";
int g_probe_capacity = 0, g_probe_count = 0, g_probe_events = 0;
hipEvent_t g_probe_start[kProbeMax], g_probe_stop[kProbeMax];
int g_probe_wgs[kProbeMax];
}  // namespace

int probe_before(const char* name, hipStream_t s) {
    if (!g_probe_armed.load(std::memory_order_relaxed)) return -1;
    if (!strstr(name, g_probe_name) || g_probe_count >= g_probe_capacity) return -1;
    const int slot = g_probe_count++;
    (void)hipEventRecord(g_probe_start[slot], s);
    return slot;
}
void probe_after(int slot, int workgroups, hipStream_t s) {
    if (slot < 0) return;
    g_probe_wgs[slot] = workgroups;
    (void)hipEventRecord(g_probe_stop[slot], s);
}


// a plain tensor whose producer writes `records` per-workgroup maxima of |value|
void carve_amax(Ctx& c, DT& t, int records) {
    t.bound = c.get<float>((size_t)records);
    t.bound_n = records;
    t.bounded = true;
}

// a caller-provided plain tensor as a source, registered on the tape when one is being recorded
Src external_src(Ctx& c, const float* p, const Geom& g, int bcast_d, bool needs_grad) {
    Src s{p, nullptr, nullptr, 0, bcast_d};
    if (c.tape) {
        TapeTensor t;
        t.raw = p;
        t.g = g;
        t.bcast_d = bcast_d;
        t.needs_grad = needs_grad;
        s.id = c.tape->add(t);
    }
    return s;
}

void tape_layer(Ctx& c, int type, int kd, int stride, const Src& a, const Src& b, const Geom& in_g, DT& o,
                       const PdsConvBlockParams* P, bool norm) {
    if (!c.tape) return;
    TapeTensor t;
    t.raw = o.raw;
    t.scale = o.scale;
    t.shift = o.shift;
    t.mean = o.mean;
    t.rstd = o.rstd;
    t.g = o.g;
    t.per_plane = o.per_plane;
    t.bound = o.bound;
    t.bound_n = o.bound_n;
    t.bounded = o.bounded;
    o.id = c.tape->add(t);
    TapeLayer L;
    L.type = type;
    L.kd = kd;
    L.stride = stride;
    L.a = a.id;
    L.b = b.p ? b.id : -1;
    L.out = o.id;
    L.in_g = in_g;
    L.out_g = o.g;
    L.P = P;
    L.norm = norm;
    c.tape->layers.push_back(L);
}

Geom conv_out_geom(const Geom& in, int cout, int kd, int stride) {
    Geom o = in;
    o.c = cout;
    if (stride == 2) {
        if (kd == 3) o.d = (in.d + 1) / 2;
        o.h = (in.h + 1) / 2;
        o.w = (in.w + 1) / 2;
    }
    return o;
}


// conv (+ LeakyReLU + deferred InstanceNorm when P.gamma) ; out_raw may be caller-provided
DT conv_block(Ctx& c, const Src& a, const Src& b, const Geom& in, const PdsConvBlockParams& P, int cout, int kd, int stride,
              int per_plane, float* out_raw, bool allow_mfma, float* scale_out, float* shift_out, const ConvExtra* extra) {
    DT o;
    o.g = conv_out_geom(in, cout, kd, stride);
    o.per_plane = per_plane;
    o.raw = out_raw ? out_raw : c.get<float>(o.g.numel());
    const bool norm = P.gamma != nullptr;
    ConvLayer L;
    L.a = a;
    L.b = b;
    L.in = in;
    L.weight = (extra && extra->s2d_cin) ? extra->weight_used : P.weight;
    L.bias = P.bias;
    L.out = o.raw;
    L.out_g = o.g;
    L.kd = kd;
    L.stride = stride;
    L.lrelu = norm ? 1 : 0;
    L.stat_per_plane = per_plane;
    L.partials = nullptr;
    L.packed = nullptr;
    L.sink = c.sink;
    if (extra) {
        L.l0A = extra->l0A;
        L.l0G = extra->l0G;
        L.l0G2 = extra->l0G2;
        L.l0_cstride = extra->l0_cstride;
        L.l0_rs = extra->l0_rs;
        L.out_batch_channels = extra->out_batch_channels;
        L.d_begin = extra->d_begin;
        L.side_out = extra->side_out;
        L.plane_weight_sets = extra->plane_weight_sets;
        L.out_cb8 = extra->out_cb8 ? 1 : 0;
        L.l1B = extra->l1B;
        L.l1H = extra->l1H;
        L.l1_bstride = extra->l1_bstride;
        L.l1_hstride = extra->l1_hstride;
        L.l1_edge = extra->l1_edge;
        L.l1_P = extra->l1_P;
        L.l1_d0 = extra->l1_d0;
    }
    o.cb8 = L.out_cb8 != 0;
    // kernel choice: 0 = direct VALU, 2 = conv2d MFMA (kd 1), 3 = conv3d MFMA (kd 3), 4 = conv2d MFMA in the
    // Winograd domain (plain single-source Cin -> 64 layers), 9 = conv2d on the bf16 pipe with three-way split operands
    int kind = 0;
    if (allow_mfma && !norm && !c.tape && conv2d_t8_supported(L)) kind = 8;   // persistent y-Toeplitz kernel, no packing
    else if (allow_mfma && !(extra && extra->matching_extras()) && conv2d_x3_supported(L)) kind = 9;
    else if (allow_mfma && conv2d_mfma_supported(L)) kind = conv2d_wino_eligible(L) ? 4 : 2;
    else if (allow_mfma && conv3d_t8_supported(L)) kind = 6;   // persistent z-Toeplitz kernel, no weight packing
    else if (allow_mfma && conv3d_ks_supported(L)) kind = 7;   // inner levels: K split over the waves
    else if (allow_mfma && conv3d_nx_supported(L)) kind = 10;  // 16-channel quarter-resolution layers: fp16-split operands
    else if (allow_mfma && conv3d_mfma_supported(L)) kind = 3;
    if (kind == 2)
        L.packed = c.get<float>(conv2d_mfma_packed_floats(in.c, cout) * (L.plane_weight_sets > 0 ? L.plane_weight_sets : 1));
    if (kind == 4)
        L.packed = c.get<float>(conv2d_wino_packed_floats(in.c, cout) * (L.plane_weight_sets > 0 ? L.plane_weight_sets : 1));
    if (kind == 3) L.packed = c.get<float>(conv3d_mfma_packed_floats(o.g, in.c, stride));
    if (kind == 7) L.packed = c.get<float>(conv3d_ks_packed_floats(in.c, cout, 27));
    if (kind == 10) L.packed = c.get<float>(conv3d_nx_packed_floats(in.c, cout));
    if (kind == 9) L.packed = c.get<float>(conv2d_x3_packed_floats(in.c));
    // (conv2d_t8 / conv2d_t8w read planar tensors only: nothing but conv2d_x3 takes or writes the blocked layout)
    if ((a.cb8 || b.cb8 || L.out_cb8) && !(kind == 9 && !b.p && conv2d_x3_cb8_ok(L, a.cb8 != 0, L.out_cb8 != 0))) {
        c.run(set_error(-1, "conv_block: a channel-blocked tensor reached a kernel that does not take it"));
        return o;
    }
    if (L.l1B && kind != 9) {
        c.run(set_error(-1, "conv_block: the on-the-fly layer-1 source needs conv2d_x3"));
        return o;
    }
    if (L.out_batch_channels && kind != 4 && kind != 9) {
        c.run(set_error(-1, "conv_block: a channel-slice output needs the Winograd kernel"));
        return o;
    }
    if (extra && extra->matching_extras() && kind != 2 && kind != 4 && kind != 8) {
        c.run(set_error(-1, "conv_block: fused Matching extras need the conv2d MFMA kernel"));
        return o;
    }
    auto launch = [&]() {
        return kind == 2 ? launch_conv2d_mfma(L, c.s)
                         : kind == 4 ? launch_conv2d_wino(L, c.s)
                                     : kind == 3 ? launch_conv3d_mfma(L, c.s)
                                                 : kind == 6 ? launch_conv3d_t8(L, c.s)
                                                             : kind == 7 ? launch_conv3d_ks(L, c.s)
                                                             : kind == 10 ? launch_conv3d_nx(L, c.s)
                                                                         : kind == 8 ? launch_conv2d_t8(L, c.s)
                                                                                     : kind == 9 ? launch_conv2d_x3(L, c.s) : launch_conv_direct(L, c.s);
    };
    const bool collecting = c.sink && c.sink->phase == kPackCollect && c.base != nullptr;
    if (collecting && kind != 0 && kind != 6 && kind != 8) c.run(launch());  // registers the pack job(s) only
    if (norm) {
        // partial records: direct / 2-D kernels write [(n, c, d)][tile]; the 3-D kernel writes [(n, c)][tile]
        const int tiles = kind == 2 ? conv2d_mfma_tiles(o.g)
                                    : kind == 4 ? conv2d_wino_tiles(o.g)
                                    : kind == 9 ? conv2d_x3_tiles(L)
                                    : kind == 3 ? conv3d_mfma_tiles(o.g, in.c, stride)
                                    : kind == 6 ? conv3d_t8_records(o.g)
                                    : kind == 7 ? conv3d_ks_tiles(o.g)
                                    : kind == 10 ? conv3d_nx_tiles(o.g) : conv_direct_tiles_for(o.g, stride);
        const bool volume_records = kind == 3 || kind == 6 || kind == 7 || kind == 10;   // [(n, c)][record] instead of [(n, c, d)][tile]
        const size_t records = (size_t)o.g.n * o.g.c * (volume_records ? 1 : o.g.d) * tiles;
        L.partials = c.get<double>(records * 2);
        const int groups = o.g.n * o.g.c * (per_plane ? o.g.d : 1);
        o.normed = true;
        o.scale = scale_out ? scale_out : c.get<float>(groups);
        o.shift = shift_out ? shift_out : c.get<float>(groups);
        o.mean = c.get<float>(groups);
        o.rstd = c.get<float>(groups);
        o.bound = c.get<float>(1);
        o.bound_n = 1;
        o.bounded = true;
        if (!c.plan) {
            const int per_group = volume_records ? tiles : tiles * (per_plane ? 1 : o.g.d);
            const double count = (double)o.g.h * o.g.w * (per_plane ? 1 : o.g.d);
            bool chained = false;
            if (c.chain && kind == 7 && !per_plane) {
                const KsChainFold fold{P.gamma, P.beta, o.scale, o.shift, o.mean, o.rstd, o.bound, groups, per_group, o.g.c, count};
                c.run(conv3d_ks_chain_add(*c.chain, L, fold, &chained));
            }
            if (!chained) {
                c.flush_chain();
                c.run(launch());
                c.run(launch_in_finalize(L.partials, groups, per_group, count, P.gamma, P.beta, o.g.c,
                                         per_plane ? o.g.d : 1, o.scale, o.shift, o.mean, o.rstd, c.s, o.bound));
            }
        }
    } else if (!c.plan) {
        c.flush_chain();
        c.run(launch());
    }
    tape_layer(c, 0, kd, stride, a, b, in, o, &P, norm);
    if (c.tape && extra && extra->s2d_cin) {  // (the pointer is null in a planning walk: test the count)
        c.tape->layers.back().weight_used = extra->weight_used;
        c.tape->layers.back().s2d_cin = extra->s2d_cin;
    }
    return o;
}

DT deconv_block(Ctx& c, const Src& a, const Src& b, const Geom& in, const PdsConvBlockParams& P, int cout, int kd,
                float* out_raw, float* scale_out, float* shift_out) {
    DT o;
    o.g = in;
    o.g.c = cout;
    o.g.d = (kd == 4) ? in.d * 2 : in.d;
    o.g.h = in.h * 2;
    o.g.w = in.w * 2;
    o.per_plane = 0;
    o.raw = out_raw ? out_raw : c.get<float>(o.g.numel());
    const bool norm = P.gamma != nullptr;
    DeconvLayer L;
    L.a = a;
    L.b = b;
    L.in = in;
    L.weight = P.weight;
    L.bias = P.bias;
    L.out = o.raw;
    L.out_g = o.g;
    L.kd = kd;
    L.lrelu = norm ? 1 : 0;
    L.partials = nullptr;
    L.packed = nullptr;
    L.sink = c.sink;
    const bool cell = deconv3d_cell_supported(L);   // persistent dense-cell kernel: no weight packing
    const bool ks = !cell && deconv3d_ks_supported(L);   // inner levels: cell form, K split over the waves
    const bool mfma = !cell && !ks && deconv3d_mfma_supported(L);
    if (mfma) L.packed = c.get<float>(deconv3d_mfma_packed_floats(in, cout, kd));
    if (ks) L.packed = c.get<float>(conv3d_ks_packed_floats(in.c, 8 * cout, 8));
    if (mfma && c.sink && c.sink->phase == kPackCollect && c.base != nullptr) c.run(launch_deconv3d_mfma(L, c.s));
    if (ks && c.sink && c.sink->phase == kPackCollect && c.base != nullptr) c.run(launch_deconv3d_ks(L, c.s));
    auto launch = [&]() {
        return cell ? launch_deconv3d_cell(L, c.s)
                    : ks ? launch_deconv3d_ks(L, c.s) : mfma ? launch_deconv3d_mfma(L, c.s) : launch_deconv_direct(L, c.s);
    };
    // partial records per (n, c): cell kernel [workgroup]; K-split / MFMA kernels [tile][parity class]; direct [d][tile]
    const int per_group = cell ? deconv3d_cell_records(in, cout)
                               : ks ? deconv3d_ks_tiles(in, cout) * 8
                                    : mfma ? deconv3d_mfma_tiles(in) * (kd == 4 ? 8 : 4) : deconv_direct_tiles(o.g) * o.g.d;
    if (norm) {
        const size_t records = (size_t)o.g.n * o.g.c * per_group;
        L.partials = c.get<double>(records * 2);
        const int groups = o.g.n * o.g.c;
        o.normed = true;
        o.scale = scale_out ? scale_out : c.get<float>(groups);
        o.shift = shift_out ? shift_out : c.get<float>(groups);
        o.mean = c.get<float>(groups);
        o.rstd = c.get<float>(groups);
        o.bound = c.get<float>(1);
        o.bound_n = 1;
        o.bounded = true;
        if (!c.plan) {
            bool chained = false;
            if (c.chain && ks) {
                const KsChainFold fold{P.gamma, P.beta, o.scale, o.shift, o.mean, o.rstd, o.bound, groups, per_group, o.g.c,
                                       (double)o.g.volume()};
                c.run(deconv3d_ks_chain_add(*c.chain, L, fold, &chained));
            }
            if (!chained) {
                c.flush_chain();
                c.run(launch());
                c.run(launch_in_finalize(L.partials, groups, per_group, (double)o.g.volume(), P.gamma, P.beta,
                                         o.g.c, 1, o.scale, o.shift, o.mean, o.rstd, c.s, o.bound));
            }
        }
    } else if (!c.plan) {
        c.flush_chain();
        c.run(launch());
    }
    tape_layer(c, 1, kd, kd == 4 ? 2 : 1, a, b, in, o, &P, norm);
    return o;
}


int check_block(const PdsConvBlockParams& b, bool norm, const char* name) {
    PDS_REQUIRE(b.weight && b.bias, "%s: null weight/bias", name);
    if (norm) PDS_REQUIRE(b.gamma && b.beta, "%s: null InstanceNorm affine", name);
    return 0;
}

}  // namespace pds

using namespace pds;

// ====================================================================================================
extern "C" {

int pds_abi_version(void) { return PDS_ABI_VERSION; }
long long pds_nonfinite_statistics(int reset) { return nonfinite_statistics(reset); }

int pds_probe_begin(const char* kernel, int capacity) {
    PDS_REQUIRE(kernel && kernel[0] && strlen(kernel) < sizeof(g_probe_name), "probe: bad kernel name");
    PDS_REQUIRE(capacity > 0 && capacity <= kProbeMax, "probe: capacity %d outside 1..%d", capacity, kProbeMax);
    for (; g_probe_events < capacity; ++g_probe_events) {
        if (hipEventCreate(&g_probe_start[g_probe_events]) != hipSuccess ||
            hipEventCreate(&g_probe_stop[g_probe_events]) != hipSuccess)
            return set_error(-1, "probe: hipEventCreate failed");
    }
    strcpy(g_probe_name, kernel);
    g_probe_capacity = capacity;
    g_probe_count = 0;
    g_probe_armed.store(1, std::memory_order_release);
    return 0;
}

int pds_probe_end(float* ms, int* workgroups, int capacity) {
    g_probe_armed.store(0, std::memory_order_release);
    const int n = g_probe_count < capacity ? g_probe_count : capacity;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(g_probe_stop[i]) != hipSuccess) return set_error(-1, "probe: hipEventSynchronize failed");
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_probe_start[i], g_probe_stop[i]) != hipSuccess)
            return set_error(-1, "probe: hipEventElapsedTime failed");
        if (ms) ms[i] = t;
        if (workgroups) workgroups[i] = g_probe_wgs[i];
    }
    return n;
}
const char* pds_last_error(void) { return g_error; }

int pds_debug_chain_stamps(unsigned* ticks, int capacity) {
    PDS_REQUIRE(ticks && capacity > 0, "chain stamps: bad arguments");
    return ks_chain_debug_stamps(ticks, capacity);
}

int pds_subpixel_map_fwd(const float* similarities, float* disparities, int batch, int planes, int height,
                         int width, int half_support_window, int disparity_step, pds_stream_t stream) {
    PDS_REQUIRE(similarities && disparities, "subpixel_map: null pointer");
    PDS_REQUIRE(batch > 0 && planes > 0 && height > 0 && width > 0, "subpixel_map: bad shape");
    PDS_REQUIRE(disparity_step >= 1 && half_support_window >= 1 && half_support_window % disparity_step == 0,
                "subpixel_map: bad window/step");
    // Python floor division of the negated window (estimator.py:66-68)
    const int hi = half_support_window / disparity_step;
    const int lo = -((half_support_window + disparity_step - 1) / disparity_step);
    return launch_subpixel_map(similarities, disparities, batch, planes, height, width, lo, hi, disparity_step,
                               (hipStream_t)stream);
}

int pds_subpixel_map_confidence_fwd(const float* similarities, float* disparities, float* confidence, int batch,
                                    int planes, int height, int width, int half_support_window, int disparity_step,
                                    pds_stream_t stream) {
    PDS_REQUIRE(similarities && disparities && confidence, "subpixel_map_confidence: null pointer");
    PDS_REQUIRE(batch > 0 && planes > 0 && height > 0 && width > 0, "subpixel_map_confidence: bad shape");
    PDS_REQUIRE(disparity_step >= 1 && half_support_window >= 1 && half_support_window % disparity_step == 0,
                "subpixel_map_confidence: bad window/step");
    const int hi = half_support_window / disparity_step;
    const int lo = -((half_support_window + disparity_step - 1) / disparity_step);
    return launch_subpixel_map(similarities, disparities, batch, planes, height, width, lo, hi, disparity_step,
                               (hipStream_t)stream, confidence);
}

int pds_shift_concat_fwd(const float* left, const float* right, float* out, int batch, int channels, int h, int w,
                         int d_begin, int d_count, pds_stream_t stream) {
    PDS_REQUIRE(left && right && out, "shift_concat: null pointer");
    PDS_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0 && d_begin >= 0 && d_count > 0,
                "shift_concat: bad shape");
    return launch_shift_concat(left, right, out, batch, channels, h, w, d_begin, d_count, (hipStream_t)stream);
}

size_t pds_conv_block_workspace_bytes(int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                                      int per_plane) {
    PdsConvBlockParams dummy{nullptr, nullptr, (const float*)1, (const float*)1};
    // sized for the chained form (input behind a deferred InstanceNorm): it may pick a kernel with more statistics
    // records per plane than the plain form, never fewer; with and without a range bound (the kernel choice -- and with
    // it the packed-weight scratch -- depends on it): the larger of the two
    size_t need = 0;
    for (int bounded = 0; bounded < 2; ++bounded) {
        Ctx c{nullptr, 0, true, nullptr};
        Src src = plain_src(nullptr);
        src.normed = 1;
        src.bounded = bounded;
        conv_block(c, src, no_src(), Geom{n, cin, d, h, w}, dummy, cout, kd, stride, per_plane, (float*)1, true,
                   (float*)1, (float*)1);
        if (c.off > need) need = c.off;
    }
    return need + 256;
}

int pds_conv_block_fwd(const PdsConvBlockParams* params, const float* x, float* raw, float* scale, float* shift,
                       int n, int cin, int cout, int d, int h, int w, int kd, int stride, int per_plane,
                       void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(params && x && raw && workspace, "conv_block: null pointer");
    PDS_REQUIRE(params->weight && params->bias, "conv_block: null weight/bias");
    PDS_REQUIRE(n > 0 && cin > 0 && cout > 0 && d > 0 && h > 0 && w > 0, "conv_block: bad shape");
    PDS_REQUIRE((kd == 1 || kd == 3) && (stride == 1 || stride == 2) && !(kd == 1 && stride == 2),
                "conv_block: unsupported kd=%d stride=%d", kd, stride);
    if (params->gamma) PDS_REQUIRE(params->beta && scale && shift, "conv_block: null InstanceNorm outputs");
    const size_t need = pds_conv_block_workspace_bytes(n, cin, cout, d, h, w, kd, stride, per_plane);
    PDS_REQUIRE(workspace_bytes >= need, "conv_block: workspace too small (%zu < %zu)", workspace_bytes, need);
    Ctx c{(char*)workspace, 0, false, (hipStream_t)stream};
    conv_block(c, plain_src(x), no_src(), Geom{n, cin, d, h, w}, *params, cout, kd, stride, per_plane, raw, true,
               scale, shift);
    return c.err;
}

// The same block behind another block: x is the producer's RAW output and the loader applies the producer's folded
// InstanceNorm, x^ = x_scale * x + x_shift (per (n, c), or per (n, c, d) when x_per_plane) -- how the blocks of
// MatchingOperation / Regularization are chained inside the modules (no normalised tensor is ever stored).  x_bound
// (one device float bounding |x^|, or null) is the range certificate of common.hpp Src::bound.
int pds_conv_block_chained_fwd(const PdsConvBlockParams* params, const float* x, const float* x_scale,
                               const float* x_shift, int x_per_plane, const float* x_bound, float* raw, float* scale,
                               float* shift, int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                               int per_plane, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(params && x && x_scale && x_shift && raw && workspace, "conv_block_chained: null pointer");
    PDS_REQUIRE(params->weight && params->bias, "conv_block_chained: null weight/bias");
    PDS_REQUIRE(n > 0 && cin > 0 && cout > 0 && d > 0 && h > 0 && w > 0, "conv_block_chained: bad shape");
    PDS_REQUIRE((kd == 1 || kd == 3) && (stride == 1 || stride == 2) && !(kd == 1 && stride == 2),
                "conv_block_chained: unsupported kd=%d stride=%d", kd, stride);
    if (params->gamma) PDS_REQUIRE(params->beta && scale && shift, "conv_block_chained: null InstanceNorm outputs");
    const size_t need = pds_conv_block_workspace_bytes(n, cin, cout, d, h, w, kd, stride, per_plane);
    PDS_REQUIRE(workspace_bytes >= need, "conv_block_chained: workspace too small (%zu < %zu)", workspace_bytes, need);
    Ctx c{(char*)workspace, 0, false, (hipStream_t)stream};
    Src src{x, x_scale, x_shift, x_per_plane ? 1 : 0, 0};
    src.normed = 1;
    if (x_bound) {
        src.bound = x_bound;
        src.bound_n = 1;
        src.bounded = 1;
    }
    conv_block(c, src, no_src(), Geom{n, cin, d, h, w}, *params, cout, kd, stride, per_plane, raw, true, scale, shift);
    return c.err;
}

// ABI v7.  One transposed block (network_blocks.py:37-44, 75-85) through deconv_block -- the dispatch of the module walks --
// on a plain source (x_scale == NULL) or behind a deferred InstanceNorm, with or without a range certificate.
size_t pds_deconv_block_workspace_bytes(int n, int cin, int cout, int d, int h, int w, int kd) {
    PdsConvBlockParams dummy{nullptr, nullptr, (const float*)1, (const float*)1};
    // as pds_conv_block_workspace_bytes: the chained form with and without a range bound, the larger of the two
    size_t need = 0;
    for (int bounded = 0; bounded < 2; ++bounded) {
        Ctx c{nullptr, 0, true, nullptr};
        Src src = plain_src(nullptr);
        src.normed = 1;
        src.bounded = bounded;
        deconv_block(c, src, no_src(), Geom{n, cin, d, h, w}, dummy, cout, kd, (float*)1, (float*)1, (float*)1);
        if (c.off > need) need = c.off;
    }
    return need + 256;
}

int pds_deconv_block_chained_fwd(const PdsConvBlockParams* params, const float* x, const float* x_scale,
                                 const float* x_shift, const float* x_bound, float* raw, float* scale, float* shift,
                                 int n, int cin, int cout, int d, int h, int w, int kd, void* workspace,
                                 size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(params && x && raw && workspace, "deconv_block_chained: null pointer");
    PDS_REQUIRE(params->weight && params->bias, "deconv_block_chained: null weight/bias");
    PDS_REQUIRE((x_scale != nullptr) == (x_shift != nullptr), "deconv_block_chained: x_scale without x_shift (or the reverse)");
    PDS_REQUIRE(x_scale || !x_bound, "deconv_block_chained: a range bound goes with a deferred InstanceNorm (x_scale)");
    PDS_REQUIRE(n > 0 && cin > 0 && cout > 0 && d > 0 && h > 0 && w > 0, "deconv_block_chained: bad shape");
    PDS_REQUIRE(kd == 3 || kd == 4, "deconv_block_chained: unsupported kd=%d (4: k4 s2, 3: k(3,4,4) s(1,2,2))", kd);
    PDS_REQUIRE((size_t)n * cout * (kd == 4 ? 2 : 1) * d * 2 * h * 2 * w <= 0x7fffffffu &&
                    (size_t)n * cin * d * h * w <= 0x7fffffffu,
                "deconv_block_chained: tensor does not fit 32-bit indices");
    if (params->gamma) PDS_REQUIRE(params->beta && scale && shift, "deconv_block_chained: null InstanceNorm outputs");
    const size_t need = pds_deconv_block_workspace_bytes(n, cin, cout, d, h, w, kd);
    PDS_REQUIRE(workspace_bytes >= need, "deconv_block_chained: workspace too small (%zu < %zu)", workspace_bytes, need);
    Ctx c{(char*)workspace, 0, false, (hipStream_t)stream};
    c.limit = workspace_bytes;
    Src src = plain_src(x);
    if (x_scale) {
        src = Src{x, x_scale, x_shift, 0, 0};
        src.normed = 1;
        if (x_bound) {
            src.bound = x_bound;
            src.bound_n = 1;
            src.bounded = 1;
        }
    }
    deconv_block(c, src, no_src(), Geom{n, cin, d, h, w}, *params, cout, kd, raw, scale, shift);
    return c.err;
}

// ---- evaluation metrics (errors.py:9-74) ---------------------------------------------------------------
size_t pds_disparity_errors_workspace_bytes(size_t count) {
    return disparity_errors_partial_doubles(count) * sizeof(double) + 256;
}

int pds_disparity_errors_fwd(const float* estimated, const float* ground_truth, size_t count, float n,
                             float* pixelwise_absolute_error, float* pixelwise_n_pixels_error, double* stats,
                             void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(estimated && ground_truth && stats && workspace, "disparity_errors: null pointer");
    PDS_REQUIRE(count > 0, "disparity_errors: empty input");
    PDS_REQUIRE(workspace_bytes >= pds_disparity_errors_workspace_bytes(count), "disparity_errors: workspace too small");
    return launch_disparity_errors(estimated, ground_truth, count, n, pixelwise_absolute_error,
                                   pixelwise_n_pixels_error, stats, reinterpret_cast<double*>(workspace),
                                   (hipStream_t)stream);
}

int pds_left_right_check_fwd(const float* left_disparity, const float* right_disparity, unsigned char* left_valid,
                             unsigned char* right_valid, float* left_filled, float* right_filled, int batch, int h,
                             int w, float max_difference, pds_stream_t stream) {
    PDS_REQUIRE(left_disparity && right_disparity && left_valid && right_valid, "left_right_check: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0 && w < (1 << 24) && (size_t)batch * h <= 0x7fffffffu,
                "left_right_check: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE(max_difference >= 0.f && max_difference <= 3.402823466e+38f,
                "left_right_check: max_difference must be finite and >= 0 (got %g)", (double)max_difference);
    PDS_REQUIRE(left_filled != left_disparity && left_filled != right_disparity && right_filled != left_disparity &&
                    right_filled != right_disparity && (!left_filled || left_filled != right_filled),
                "left_right_check: a filled output aliases an input");
    return launch_left_right_check(left_disparity, right_disparity, left_valid, right_valid, left_filled, right_filled,
                                   batch * h, w, max_difference, (hipStream_t)stream);
}

// (shared by the query and the entry point; 0: refused, the message is set)
static size_t speckle_checked_bytes(int batch, int h, int w) {
    if (!(batch > 0 && h > 0 && w > 0)) {
        set_error(-1, "speckle_filter: bad shape (%d, %d, %d)", batch, h, w);
        return 0;
    }
    if ((size_t)h * w > 0x7fffffffu) {
        set_error(-1, "speckle_filter: an image of %d x %d pixels does not fit 32-bit labels", h, w);
        return 0;
    }
    if ((size_t)batch * h * w > speckle_max_pixels()) {
        set_error(-1, "speckle_filter: batch * h * w = %zu does not fit 32-bit indices (at most %zu)",
                  (size_t)batch * h * w, speckle_max_pixels());
        return 0;
    }
    return speckle_workspace_bytes(batch, h, w);
}

size_t pds_speckle_filter_workspace_bytes(int batch, int h, int w) { return speckle_checked_bytes(batch, h, w); }

int pds_speckle_filter_fwd(const float* disparity, const unsigned char* valid, unsigned char* keep, float* filtered,
                           int* sizes, int batch, int h, int w, float max_difference, int max_size, float fill_value,
                           void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(disparity && keep && workspace, "speckle_filter: null pointer");
    const size_t need = speckle_checked_bytes(batch, h, w);
    if (need == 0) return -1;
    PDS_REQUIRE(max_difference >= 0.f && max_difference <= 3.402823466e+38f,
                "speckle_filter: max_difference must be finite and >= 0 (got %g)", (double)max_difference);
    PDS_REQUIRE(max_size >= 0, "speckle_filter: max_size must be >= 0 (got %d)", max_size);
    PDS_REQUIRE(workspace_bytes >= need, "speckle_filter: workspace too small (%zu < %zu)", workspace_bytes, need);
    // filtered may BE disparity (a pixel is read and written by the same thread of the last pass); any other overlap of
    // an output with an input or with another output is refused
    const size_t count = (size_t)batch * h * w;
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    PDS_REQUIRE(filtered == disparity || !overlap(filtered, count * 4, disparity, count * 4),
                "speckle_filter: filtered overlaps disparity without being the same buffer");
    PDS_REQUIRE(!overlap(keep, count, disparity, count * 4) && !overlap(keep, count, valid, count) &&
                    !overlap(sizes, count * 4, disparity, count * 4) && !overlap(sizes, count * 4, valid, count) &&
                    !overlap(filtered, count * 4, valid, count) && !overlap(keep, count, filtered, count * 4) &&
                    !overlap(keep, count, sizes, count * 4) && !overlap(sizes, count * 4, filtered, count * 4),
                "speckle_filter: an output aliases an input or another output");
    return launch_speckle_filter(disparity, valid, keep, filtered, sizes, batch, h, w, max_difference, max_size,
                                 fill_value, workspace, (hipStream_t)stream);
}

int pds_median_filter_fwd(const float* disparity, const unsigned char* valid, float* filtered, unsigned char* ok,
                          int batch, int h, int w, int kernel_size, int fill_holes, int min_valid, float fill_value,
                          pds_stream_t stream) {
    PDS_REQUIRE(disparity && filtered, "median_filter: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0, "median_filter: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu, "median_filter: batch * h * w = %zu does not fit 32-bit indices",
                (size_t)batch * h * w);
    PDS_REQUIRE(kernel_size == 3 || kernel_size == 5 || kernel_size == 7,
                "median_filter: kernel_size must be 3, 5 or 7 (got %d)", kernel_size);
    PDS_REQUIRE(min_valid >= 1 && min_valid <= kernel_size * kernel_size,
                "median_filter: min_valid must be in 1 .. %d (got %d)", kernel_size * kernel_size, min_valid);
    // neighbours are read: no output may overlap an input, nor the other output
    const size_t count = (size_t)batch * h * w;
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    PDS_REQUIRE(!overlap(filtered, count * 4, disparity, count * 4), "median_filter: filtered overlaps disparity");
    PDS_REQUIRE(!overlap(ok, count, valid, count), "median_filter: ok overlaps valid");
    PDS_REQUIRE(!overlap(filtered, count * 4, valid, count) && !overlap(ok, count, disparity, count * 4) &&
                    !overlap(ok, count, filtered, count * 4),
                "median_filter: an output aliases an input or the other output");
    return launch_median_filter(disparity, valid, filtered, ok, batch, h, w, kernel_size, fill_holes != 0, min_valid,
                                fill_value, (hipStream_t)stream);
}

int pds_rectify_maps_fwd(const double* inverse_projection, const double* camera, const double* distortion,
                         float* map_x, float* map_y, int h, int w, pds_stream_t stream) {
    PDS_REQUIRE(inverse_projection && camera && distortion && map_x && map_y, "rectify_maps: null pointer");
    PDS_REQUIRE(h > 0 && w > 0 && h < (1 << 24) && w < (1 << 24) && (size_t)h * w <= 0x7fffffffu,
                "rectify_maps: bad shape (%d, %d)", h, w);
    PDS_REQUIRE(map_x != map_y, "rectify_maps: map_x aliases map_y");
    RectifyMapsArgs a;
    for (int k = 0; k < 9; ++k) a.inverse_projection[k] = inverse_projection[k];
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        a.distortion[k] = distortion[k];
    }
    for (int k = 0; k < 9; ++k) PDS_REQUIRE(std::isfinite(a.inverse_projection[k]), "rectify_maps: non-finite matrix");
    for (int k = 0; k < 5; ++k)
        PDS_REQUIRE(std::isfinite(a.camera[k]) && std::isfinite(a.distortion[k]),
                    "rectify_maps: non-finite camera or distortion");
    return launch_rectify_maps(a, map_x, map_y, h, w, (hipStream_t)stream);
}

int pds_remap_fwd(const void* image, int layout, const float* map_x, const float* map_y, float* out, int batch,
                  int h_in, int w_in, int h_out, int w_out, float border_value, int reverse_channels,
                  pds_stream_t stream) {
    PDS_REQUIRE(image && map_x && map_y && out, "remap: null pointer");
    PDS_REQUIRE(layout == 0 || layout == 1, "remap: bad layout %d (0: float32 NCHW, 1: uint8 NHWC)", layout);
    PDS_REQUIRE(batch > 0 && h_in > 0 && w_in > 0 && h_out > 0 && w_out > 0 && h_in < (1 << 24) && w_in < (1 << 24) &&
                    (size_t)batch * 3 * h_in * w_in <= 0x7fffffffu && (size_t)batch * 3 * h_out * w_out <= 0x7fffffffu,
                "remap: bad shape (batch %d, in %d x %d, out %d x %d)", batch, h_in, w_in, h_out, w_out);
    PDS_REQUIRE(std::isfinite(border_value), "remap: border_value must be finite (got %g)", (double)border_value);
    PDS_REQUIRE((const void*)out != image && out != map_x && out != map_y, "remap: out aliases an input");
    return launch_remap(image, layout, map_x, map_y, out, batch, h_in, w_in, h_out, w_out, border_value,
                        reverse_channels != 0, (hipStream_t)stream);
}

int pds_reproject_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                      float min_confidence, const float* matrix, float* points, float* depth, int batch, int h, int w,
                      pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix, "reproject: null pointer");
    PDS_REQUIRE(points || depth, "reproject: points and depth are both null");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0 && (size_t)batch * h * w * 3 <= 0x7fffffffu,
                "reproject: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE(!std::isnan(min_confidence), "reproject: min_confidence is NaN");
    PDS_REQUIRE(points != disparity && depth != disparity && (!points || points != depth),
                "reproject: an output aliases an input");
    ReprojectArgs a;
    for (int k = 0; k < 16; ++k) {
        a.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.matrix[k]), "reproject: non-finite matrix");
    }
    a.min_confidence = min_confidence;
    a.first = 0;
    return launch_reproject(a, disparity, valid, confidence, points, depth, batch * h * w, h, w, (hipStream_t)stream);
}

// (shared by the query and the entry point; 0: refused, the message is set)
static size_t point_cloud_checked_bytes(int batch, int h, int w) {
    if (!(batch > 0 && h > 0 && w > 0)) {
        set_error(-1, "point_cloud: bad shape (%d, %d, %d)", batch, h, w);
        return 0;
    }
    if ((size_t)batch * h * w > 0x7fffffffu) {
        set_error(-1, "point_cloud: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
        return 0;
    }
    return point_cloud_workspace_bytes((long long)batch * h * w);
}

size_t pds_point_cloud_workspace_bytes(int batch, int h, int w) { return point_cloud_checked_bytes(batch, h, w); }

int pds_point_cloud_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                        float min_confidence, const float* matrix, float min_depth, float max_depth, const void* image,
                        int image_layout, float* points, void* colors, int* index, int* offsets, long long capacity,
                        int batch, int h, int w, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix && points && offsets && workspace, "point_cloud: null pointer");
    const size_t need = point_cloud_checked_bytes(batch, h, w);
    if (need == 0) return -1;
    PDS_REQUIRE(capacity >= 0, "point_cloud: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(!colors || image, "point_cloud: colors without an image");
    PDS_REQUIRE(!image || image_layout == 0 || image_layout == 1,
                "point_cloud: bad image_layout %d (0: float32 NCHW, 1: uint8 NHWC)", image_layout);
    PDS_REQUIRE(workspace_bytes >= need, "point_cloud: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!std::isnan(min_confidence), "point_cloud: min_confidence is NaN");
    PDS_REQUIRE(!std::isnan(min_depth) && !std::isnan(max_depth), "point_cloud: a depth bound is NaN");
    PDS_REQUIRE(min_depth <= max_depth, "point_cloud: min_depth %g > max_depth %g", (double)min_depth,
                (double)max_depth);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)points & 3u) == 0 && ((uintptr_t)index & 3u) == 0 &&
                    ((uintptr_t)offsets & 3u) == 0 && ((uintptr_t)workspace & 3u) == 0 &&
                    (image_layout != 0 || (((uintptr_t)image & 3u) == 0 && ((uintptr_t)colors & 3u) == 0)),
                "point_cloud: a 32-bit buffer is not 4-byte aligned");
    // the scatter pass reads the inputs again after rows have been written: no output may overlap an input or another
    // output
    const size_t count = (size_t)batch * h * w, rows = (size_t)capacity;
    const size_t image_bytes = image ? count * (image_layout == 1 ? 3 : 12) : 0;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4},
                                                          {image, image_bytes}},
                                                  out[] = {{points, rows * 12},
                                                           {colors, rows * (image_layout == 1 ? 3 : 12)},
                                                           {index, rows * 4},
                                                           {offsets, ((size_t)batch + 1) * 4},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "point_cloud: an output aliases an input");
        for (int j = i + 1; j < 5; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "point_cloud: an output aliases another output");
    }
    ReprojectArgs a;
    for (int k = 0; k < 16; ++k) {
        a.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.matrix[k]), "point_cloud: non-finite matrix");
    }
    a.min_confidence = min_confidence;
    a.first = 0;
    return launch_point_cloud(a, min_depth, max_depth, disparity, valid, confidence, colors ? image : nullptr,
                              image_layout, points, colors, index, offsets, capacity, batch, h, w, workspace,
                              (hipStream_t)stream);
}

// (shared by the query and the entry point; 0: refused, the message is set)
static size_t triangle_mesh_checked_bytes(int batch, int h, int w) {
    if (!(batch > 0 && h > 0 && w > 0)) {
        set_error(-1, "triangle_mesh: bad shape (%d, %d, %d)", batch, h, w);
        return 0;
    }
    if ((size_t)batch * h * w > 0x7fffffffu / 2) {
        set_error(-1, "triangle_mesh: 2 * batch * h * w = %zu does not fit 32-bit indices", 2 * (size_t)batch * h * w);
        return 0;
    }
    return triangle_mesh_workspace_bytes((long long)batch * h * w);
}

size_t pds_triangle_mesh_workspace_bytes(int batch, int h, int w) { return triangle_mesh_checked_bytes(batch, h, w); }

int pds_triangle_mesh_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                          float min_confidence, const float* matrix, float min_depth, float max_depth,
                          float max_difference, int flip, const void* image, int image_layout, float* points,
                          void* colors, int* index, int* offsets, long long capacity, int* faces, int* face_offsets,
                          long long face_capacity, int batch, int h, int w, void* workspace, size_t workspace_bytes,
                          pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix && points && offsets && faces && face_offsets && workspace,
                "triangle_mesh: null pointer");
    const size_t need = triangle_mesh_checked_bytes(batch, h, w);
    if (need == 0) return -1;
    PDS_REQUIRE(capacity >= 0, "triangle_mesh: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(face_capacity >= 0, "triangle_mesh: face_capacity must be >= 0 (got %lld)", face_capacity);
    PDS_REQUIRE(!colors || image, "triangle_mesh: colors without an image");
    PDS_REQUIRE(!image || image_layout == 0 || image_layout == 1,
                "triangle_mesh: bad image_layout %d (0: float32 NCHW, 1: uint8 NHWC)", image_layout);
    PDS_REQUIRE(workspace_bytes >= need, "triangle_mesh: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!std::isnan(min_confidence), "triangle_mesh: min_confidence is NaN");
    PDS_REQUIRE(!std::isnan(min_depth) && !std::isnan(max_depth), "triangle_mesh: a depth bound is NaN");
    PDS_REQUIRE(min_depth <= max_depth, "triangle_mesh: min_depth %g > max_depth %g", (double)min_depth,
                (double)max_depth);
    PDS_REQUIRE(max_difference >= 0.f, "triangle_mesh: max_difference must be >= 0 and not NaN (got %g)",
                (double)max_difference);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)points & 3u) == 0 && ((uintptr_t)index & 3u) == 0 &&
                    ((uintptr_t)offsets & 3u) == 0 && ((uintptr_t)faces & 3u) == 0 &&
                    ((uintptr_t)face_offsets & 3u) == 0 &&
                    (image_layout != 0 || (((uintptr_t)image & 3u) == 0 && ((uintptr_t)colors & 3u) == 0)),
                "triangle_mesh: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 15u) == 0, "triangle_mesh: workspace is not 16-byte aligned");
    // the scatter passes read the inputs again after rows have been written: no output may overlap an input or another
    // output
    const size_t count = (size_t)batch * h * w, rows = (size_t)capacity;
    const size_t image_bytes = image ? count * (image_layout == 1 ? 3 : 12) : 0;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4},
                                                          {image, image_bytes}},
                                                  out[] = {{points, rows * 12},
                                                           {colors, rows * (image_layout == 1 ? 3 : 12)},
                                                           {index, rows * 4},
                                                           {offsets, ((size_t)batch + 1) * 4},
                                                           {faces, (size_t)face_capacity * 12},
                                                           {face_offsets, ((size_t)batch + 1) * 4},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 7; ++i) {
        for (int j = 0; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "triangle_mesh: an output aliases an input");
        for (int j = i + 1; j < 7; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "triangle_mesh: an output aliases another output");
    }
    ReprojectArgs a;
    for (int k = 0; k < 16; ++k) {
        a.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.matrix[k]), "triangle_mesh: non-finite matrix");
    }
    a.min_confidence = min_confidence;
    a.first = 0;
    return launch_triangle_mesh(a, min_depth, max_depth, max_difference, flip, disparity, valid, confidence,
                                colors ? image : nullptr, image_layout, points, colors, index, offsets, capacity, faces,
                                face_offsets, face_capacity, batch, h, w, workspace, (hipStream_t)stream);
}

// (shared by the query and the entry point; 0: refused, the message is set)
static size_t register_depth_checked_bytes(int batch, int ht, int wt) {
    if (!(batch > 0 && ht > 0 && wt > 0)) {
        set_error(-1, "register_depth: bad target shape (%d, %d, %d)", batch, ht, wt);
        return 0;
    }
    if ((size_t)ht * wt > 0x7fffffffu || (size_t)batch * ht * wt > 0x7fffffffu) {
        set_error(-1, "register_depth: batch * ht * wt = %zu does not fit 32-bit indices", (size_t)batch * ht * wt);
        return 0;
    }
    return register_depth_workspace_bytes((long long)batch * ht * wt);
}

size_t pds_register_depth_workspace_bytes(int batch, int ht, int wt) {
    return register_depth_checked_bytes(batch, ht, wt);
}

int pds_register_depth_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                           float min_confidence, const float* matrix, const float* camera, const float* distortion,
                           int splat, float fill_value, float* depth, int* index, unsigned char* valid_out, int batch,
                           int h, int w, int ht, int wt, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix && camera && distortion && depth && workspace, "register_depth: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0, "register_depth: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE((size_t)h * w <= 0x7fffffffu && (size_t)batch * h * w <= 0x7fffffffu,
                "register_depth: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
    const size_t need = register_depth_checked_bytes(batch, ht, wt);
    if (need == 0) return -1;
    PDS_REQUIRE(splat == 1 || splat == 2, "register_depth: splat must be 1 or 2 (got %d)", splat);
    PDS_REQUIRE(workspace_bytes >= need, "register_depth: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(std::isfinite(min_confidence), "register_depth: min_confidence must be finite (got %g)",
                (double)min_confidence);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 && ((uintptr_t)depth & 3u) == 0 &&
                    ((uintptr_t)index & 3u) == 0,
                "register_depth: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 7u) == 0, "register_depth: workspace is not 8-byte aligned");
    // the scatter reads the inputs while keys are written, the resolve writes while keys are read: nothing written may
    // overlap anything read or written
    const size_t count = (size_t)batch * h * w, targets = (size_t)batch * ht * wt;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4}},
                                                  out[] = {{depth, targets * 4},
                                                           {index, targets * 4},
                                                           {valid_out, targets},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "register_depth: an output aliases an input");
        for (int j = i + 1; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "register_depth: an output aliases another output");
    }
    RegisterDepthArgs a;
    for (int k = 0; k < 16; ++k) {
        a.r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.r.matrix[k]), "register_depth: non-finite matrix");
    }
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        a.distortion[k] = distortion[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]) && std::isfinite(a.distortion[k]),
                    "register_depth: non-finite camera or distortion");
    }
    a.r.min_confidence = min_confidence;
    a.r.first = 0;
    a.fill_value = fill_value;
    a.splat = splat;
    return launch_register_depth(a, disparity, valid, confidence, depth, index, valid_out, batch, h, w, ht, wt,
                                 workspace, (hipStream_t)stream);
}

int pds_surface_normals_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                            float min_confidence, const float* matrix, const float* viewpoint, int kernel_size,
                            float max_difference, int min_valid, float fill_value, float* normals,
                            unsigned char* valid_out, int batch, int h, int w, pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix && normals, "surface_normals: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0, "surface_normals: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu,
                "surface_normals: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
    PDS_REQUIRE(kernel_size == 3 || kernel_size == 5 || kernel_size == 7,
                "surface_normals: kernel_size must be 3, 5 or 7 (got %d)", kernel_size);
    PDS_REQUIRE(min_valid >= 3 && min_valid <= kernel_size * kernel_size,
                "surface_normals: min_valid must be in 3 .. %d (got %d)", kernel_size * kernel_size, min_valid);
    PDS_REQUIRE(max_difference >= 0.f, "surface_normals: max_difference must be >= 0 and not NaN (got %g)",
                (double)max_difference);
    PDS_REQUIRE(std::isfinite(min_confidence), "surface_normals: min_confidence must be finite (got %g)",
                (double)min_confidence);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 && ((uintptr_t)normals & 3u) == 0,
                "surface_normals: a 32-bit buffer is not 4-byte aligned");
    // neighbours are read while records are written: no output may overlap an input or the other output
    const size_t count = (size_t)batch * h * w;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4}},
                                                  out[] = {{normals, count * 12}, {valid_out, count}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "surface_normals: an output aliases an input");
    PDS_REQUIRE(!overlap(out[0].p, out[0].bytes, out[1].p, out[1].bytes),
                "surface_normals: an output aliases another output");
    SurfaceNormalsArgs a;
    for (int k = 0; k < 16; ++k) {
        a.r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.r.matrix[k]), "surface_normals: non-finite matrix");
    }
    for (int k = 0; k < 3; ++k) {
        a.viewpoint[k] = viewpoint ? viewpoint[k] : 0.f;
        PDS_REQUIRE(std::isfinite(a.viewpoint[k]), "surface_normals: non-finite viewpoint");
    }
    a.r.min_confidence = min_confidence;
    a.r.first = 0;
    a.max_difference = max_difference;
    a.fill_value = fill_value;
    a.min_valid = min_valid;
    return launch_surface_normals(a, disparity, valid, confidence, normals, valid_out, batch, h, w, kernel_size,
                                  (hipStream_t)stream);
}

// (shared by the queries and the entry points; false: refused, the message is set)
static bool tsdf_volume_ok(int nx, int ny, int nz) {
    if (!(nx > 0 && ny > 0 && nz > 0)) {
        set_error(-1, "tsdf: bad volume (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    if (nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24)) {   // (the kernels take voxel indices as exact floats)
        set_error(-1, "tsdf: a dimension above 2^24 (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    if ((size_t)nx * ny > 0x7fffffffu || (size_t)nx * ny * nz > 0x7fffffffu / 3) {
        set_error(-1, "tsdf: 3 * nx * ny * nz does not fit 32-bit indices (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    return true;
}

static size_t tsdf_integrate_checked_bytes(int h, int w) {
    if (!(h > 0 && w > 0)) {
        set_error(-1, "tsdf_integrate: bad shape (%d, %d)", h, w);
        return 0;
    }
    if ((size_t)h * w > 0x7fffffffu) {
        set_error(-1, "tsdf_integrate: h * w = %zu does not fit 32-bit indices", (size_t)h * w);
        return 0;
    }
    return tsdf_integrate_workspace_bytes((long long)h * w);
}

size_t pds_tsdf_integrate_workspace_bytes(int h, int w) { return tsdf_integrate_checked_bytes(h, w); }

int pds_tsdf_integrate_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                           float min_confidence, int weight_by_confidence, const float* matrix, const float* transforms,
                           const float* camera, float truncation, float max_weight, float* tsdf, float* weight, int nx,
                           int ny, int nz, int batch, int h, int w, void* workspace, size_t workspace_bytes,
                           pds_stream_t stream) {
    PDS_REQUIRE(disparity && matrix && transforms && camera && tsdf && weight && workspace, "tsdf_integrate: null pointer");
    PDS_REQUIRE(batch > 0, "tsdf_integrate: bad batch %d", batch);
    const size_t need = tsdf_integrate_checked_bytes(h, w);
    if (need == 0) return -1;
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu, "tsdf_integrate: batch * h * w = %zu does not fit 32-bit indices",
                (size_t)batch * h * w);
    if (!tsdf_volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(workspace_bytes >= need, "tsdf_integrate: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!weight_by_confidence || confidence, "tsdf_integrate: weight_by_confidence without a confidence");
    PDS_REQUIRE(std::isfinite(min_confidence), "tsdf_integrate: min_confidence must be finite (got %g)",
                (double)min_confidence);
    PDS_REQUIRE(truncation > 0.f && std::isfinite(truncation), "tsdf_integrate: truncation must be positive and finite (got %g)",
                (double)truncation);
    PDS_REQUIRE(max_weight > 0.f, "tsdf_integrate: max_weight must be positive (got %g)", (double)max_weight);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 && ((uintptr_t)tsdf & 3u) == 0 &&
                    ((uintptr_t)weight & 3u) == 0,
                "tsdf_integrate: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 15u) == 0, "tsdf_integrate: workspace is not 16-byte aligned");
    // the volume is read and written while the inputs and the workspace are read: nothing written may overlap anything
    const size_t count = (size_t)batch * h * w, voxels = (size_t)nx * ny * nz;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4}},
                                                  out[] = {{tsdf, voxels * 4}, {weight, voxels * 4}, {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "tsdf_integrate: the volume or the workspace aliases an input");
        for (int j = i + 1; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_integrate: tsdf, weight and the workspace alias one another");
    }
    ReprojectArgs r;
    for (int k = 0; k < 16; ++k) {
        r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(r.matrix[k]), "tsdf_integrate: non-finite matrix");
    }
    r.min_confidence = min_confidence;
    r.first = 0;
    for (size_t k = 0; k < 12 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(transforms[k]), "tsdf_integrate: non-finite transform");
    TsdfIntegrateArgs a = {};   // (A and b: per entry, from `transforms`)
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "tsdf_integrate: non-finite camera");
    }
    a.truncation = truncation;
    a.max_weight = max_weight;
    return launch_tsdf_integrate(r, a, transforms, weight_by_confidence, disparity, valid, confidence, tsdf, weight, nx,
                                 ny, nz, batch, h, w, workspace, (hipStream_t)stream);
}

size_t pds_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    return tsdf_volume_ok(nx, ny, nz) ? tsdf_extract_workspace_bytes((long long)nx * ny * nz) : 0;
}

int pds_tsdf_extract_fwd(const float* tsdf, const float* weight, const float* origin, float voxel_size,
                         float min_weight, float* points, float* normals, int* index, int* offsets, long long capacity,
                         int nx, int ny, int nz, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(tsdf && weight && origin && points && offsets && workspace, "tsdf_extract: null pointer");
    const size_t need = pds_tsdf_extract_workspace_bytes(nx, ny, nz);
    if (need == 0) return -1;
    PDS_REQUIRE(capacity >= 0, "tsdf_extract: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(workspace_bytes >= need, "tsdf_extract: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(voxel_size > 0.f && std::isfinite(voxel_size), "tsdf_extract: voxel_size must be positive and finite (got %g)",
                (double)voxel_size);
    PDS_REQUIRE(!std::isnan(min_weight), "tsdf_extract: min_weight is NaN");
    PDS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
                "tsdf_extract: non-finite origin");
    PDS_REQUIRE(((uintptr_t)tsdf & 3u) == 0 && ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)points & 3u) == 0 &&
                    ((uintptr_t)normals & 3u) == 0 && ((uintptr_t)index & 3u) == 0 && ((uintptr_t)offsets & 3u) == 0 &&
                    ((uintptr_t)workspace & 3u) == 0,
                "tsdf_extract: a 32-bit buffer is not 4-byte aligned");
    // the scatter pass reads the volume again after rows have been written: no output may overlap an input or another
    // output
    const size_t voxels = (size_t)nx * ny * nz, rows = (size_t)capacity;
    const struct { const void* p; size_t bytes; } in[] = {{tsdf, voxels * 4}, {weight, voxels * 4}},
                                                  out[] = {{points, rows * 12},
                                                           {normals, rows * 12},
                                                           {index, rows * 4},
                                                           {offsets, 8},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 2; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "tsdf_extract: an output aliases an input");
        for (int j = i + 1; j < 5; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_extract: an output aliases another output");
    }
    return launch_tsdf_extract(tsdf, weight, origin, voxel_size, min_weight, points, normals, index, offsets, capacity, nx,
                               ny, nz, workspace, (hipStream_t)stream);
}

size_t pds_tsdf_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (!tsdf_volume_ok(nx, ny, nz)) return 0;
    const size_t voxels = (size_t)nx * ny * nz, cells = (size_t)(nx - 1) * (ny - 1) * (nz - 1);
    if (voxels > 0x7fffffffu / 7) {
        set_error(-1, "tsdf_mesh: 7 * nx * ny * nz does not fit 32-bit indices (%d, %d, %d)", nx, ny, nz);
        return 0;
    }
    if (cells > 0x7fffffffu / 12) {
        set_error(-1, "tsdf_mesh: 12 * cells does not fit 32-bit indices (%d, %d, %d)", nx, ny, nz);
        return 0;
    }
    return tsdf_mesh_workspace_bytes((long long)voxels);
}

int pds_tsdf_mesh_fwd(const float* tsdf, const float* weight, const float* origin, float voxel_size, float min_weight,
                      float* points, float* normals, int* index, int* offsets, long long capacity, int* faces,
                      int* face_offsets, long long face_capacity, int nx, int ny, int nz, void* workspace,
                      size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(tsdf && weight && origin && points && offsets && faces && face_offsets && workspace,
                "tsdf_mesh: null pointer");
    const size_t need = pds_tsdf_mesh_workspace_bytes(nx, ny, nz);
    if (need == 0) return -1;
    PDS_REQUIRE(capacity >= 0, "tsdf_mesh: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(face_capacity >= 0, "tsdf_mesh: face_capacity must be >= 0 (got %lld)", face_capacity);
    PDS_REQUIRE(workspace_bytes >= need, "tsdf_mesh: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(voxel_size > 0.f && std::isfinite(voxel_size), "tsdf_mesh: voxel_size must be positive and finite (got %g)",
                (double)voxel_size);
    PDS_REQUIRE(!std::isnan(min_weight), "tsdf_mesh: min_weight is NaN");
    PDS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
                "tsdf_mesh: non-finite origin");
    PDS_REQUIRE(((uintptr_t)tsdf & 3u) == 0 && ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)points & 3u) == 0 &&
                    ((uintptr_t)normals & 3u) == 0 && ((uintptr_t)index & 3u) == 0 && ((uintptr_t)offsets & 3u) == 0 &&
                    ((uintptr_t)faces & 3u) == 0 && ((uintptr_t)face_offsets & 3u) == 0,
                "tsdf_mesh: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 15u) == 0, "tsdf_mesh: workspace is not 16-byte aligned");
    // the scatter passes read the volume and the workspace again after rows have been written: no output may overlap an
    // input or another output
    const size_t voxels = (size_t)nx * ny * nz, rows = (size_t)capacity, face_rows = (size_t)face_capacity;
    const struct { const void* p; size_t bytes; } in[] = {{tsdf, voxels * 4}, {weight, voxels * 4}},
                                                  out[] = {{points, rows * 12},     {normals, rows * 12},
                                                           {index, rows * 4},       {offsets, 8},
                                                           {faces, face_rows * 12}, {face_offsets, 8},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 7; ++i) {
        for (int j = 0; j < 2; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "tsdf_mesh: an output aliases an input");
        for (int j = i + 1; j < 7; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_mesh: an output aliases another output");
    }
    return launch_tsdf_mesh(tsdf, weight, origin, voxel_size, min_weight, points, normals, index, offsets, capacity, faces,
                            face_offsets, face_capacity, nx, ny, nz, workspace, (hipStream_t)stream);
}

int pds_tsdf_raycast_fwd(const float* tsdf, const float* weight, int nx, int ny, int nz, float voxel_size,
                         const float* rays, const float* rotations, const float* camera, float step, float z_near,
                         float z_far, float min_weight, float* depth, float* normals, int batch, int h, int w,
                         pds_stream_t stream) {
    PDS_REQUIRE(tsdf && weight && rays && rotations && camera && depth, "tsdf_raycast: null pointer");
    if (!tsdf_volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(batch > 0, "tsdf_raycast: bad batch %d", batch);
    PDS_REQUIRE(h > 0 && w > 0, "tsdf_raycast: bad shape (%d, %d)", h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu, "tsdf_raycast: batch * h * w = %zu does not fit 32-bit indices",
                (size_t)batch * h * w);
    PDS_REQUIRE(voxel_size > 0.f && std::isfinite(voxel_size), "tsdf_raycast: voxel_size must be positive and finite (got %g)",
                (double)voxel_size);
    PDS_REQUIRE(step > 0.f && std::isfinite(step), "tsdf_raycast: step must be positive and finite (got %g)", (double)step);
    PDS_REQUIRE(z_near >= 0.f && std::isfinite(z_near), "tsdf_raycast: near must be >= 0 and finite (got %g)", (double)z_near);
    PDS_REQUIRE(z_far > z_near, "tsdf_raycast: far must be above near (got %g, near %g)", (double)z_far, (double)z_near);
    PDS_REQUIRE(!std::isnan(min_weight), "tsdf_raycast: min_weight is NaN");
    // no ray is longer than the box diagonal, and |dir| >= 1: a mistyped step may not occupy the device
    const double diagonal = (double)voxel_size * std::sqrt((double)(nx - 1) * (nx - 1) + (double)(ny - 1) * (ny - 1) +
                                                           (double)(nz - 1) * (nz - 1));
    PDS_REQUIRE(diagonal / (double)step <= 65536.0,
                "tsdf_raycast: the box diagonal of %g m holds %g samples of step %g (at most 65536)", diagonal,
                diagonal / (double)step, (double)step);
    TsdfRaycastArgs a = {};
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "tsdf_raycast: non-finite camera");
    }
    PDS_REQUIRE(a.camera[0] > 0.f && a.camera[1] > 0.f, "tsdf_raycast: focal lengths must be positive (got %g, %g)",
                (double)a.camera[0], (double)a.camera[1]);
    for (size_t k = 0; k < 12 * (size_t)batch; ++k) PDS_REQUIRE(std::isfinite(rays[k]), "tsdf_raycast: non-finite ray");
    for (size_t k = 0; k < 9 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(rotations[k]), "tsdf_raycast: non-finite rotation");
    PDS_REQUIRE(((uintptr_t)tsdf & 3u) == 0 && ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)depth & 3u) == 0 &&
                    ((uintptr_t)normals & 3u) == 0,
                "tsdf_raycast: a 32-bit buffer is not 4-byte aligned");
    // the volume is read while the maps are written
    const size_t voxels = (size_t)nx * ny * nz, count = (size_t)batch * h * w;
    const struct { const void* p; size_t bytes; } in[] = {{tsdf, voxels * 4}, {weight, voxels * 4}},
                                                  out[] = {{depth, count * 4}, {normals, count * 12}};
    const auto overlap = [](const void* x, size_t xbytes, const void* y, size_t ybytes) {
        const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
        return x && y && p < q + ybytes && q < p + xbytes;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "tsdf_raycast: an output aliases the volume");
    PDS_REQUIRE(!overlap(out[0].p, out[0].bytes, out[1].p, out[1].bytes), "tsdf_raycast: an output aliases another output");
    a.step = step;
    a.z_near = z_near;
    a.z_far = z_far;
    a.min_weight = min_weight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.h = h;
    a.w = w;
    a.tiles_x = (w + kTsdfRaycastTile - 1) / kTsdfRaycastTile;
    a.tiles_y = (h + kTsdfRaycastTile - 1) / kTsdfRaycastTile;
    return launch_tsdf_raycast(a, rays, rotations, tsdf, weight, depth, normals, batch, (hipStream_t)stream);
}

int pds_tsdf_color_integrate_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                                 float min_confidence, int weight_by_confidence, const void* image, int image_layout,
                                 const float* matrix, const float* transforms, const float* camera, float truncation,
                                 float max_weight, float* tsdf, float* weight, float* color, int nx, int ny, int nz,
                                 int batch, int h, int w, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(disparity && image && matrix && transforms && camera && tsdf && weight && color && workspace,
                "tsdf_color_integrate: null pointer");
    PDS_REQUIRE(batch > 0, "tsdf_color_integrate: bad batch %d", batch);
    PDS_REQUIRE(h > 0 && w > 0, "tsdf_color_integrate: bad shape (%d, %d)", h, w);
    PDS_REQUIRE((size_t)h * w <= 0x7fffffffu, "tsdf_color_integrate: h * w = %zu does not fit 32-bit indices",
                (size_t)h * w);
    const size_t need = tsdf_integrate_workspace_bytes((long long)h * w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu,
                "tsdf_color_integrate: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
    if (!tsdf_volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(image_layout == 0 || image_layout == 1,
                "tsdf_color_integrate: image_layout must be 0 (float32 NCHW) or 1 (uint8 NHWC), got %d", image_layout);
    PDS_REQUIRE(workspace_bytes >= need, "tsdf_color_integrate: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!weight_by_confidence || confidence, "tsdf_color_integrate: weight_by_confidence without a confidence");
    PDS_REQUIRE(std::isfinite(min_confidence), "tsdf_color_integrate: min_confidence must be finite (got %g)",
                (double)min_confidence);
    PDS_REQUIRE(truncation > 0.f && std::isfinite(truncation),
                "tsdf_color_integrate: truncation must be positive and finite (got %g)", (double)truncation);
    PDS_REQUIRE(max_weight > 0.f, "tsdf_color_integrate: max_weight must be positive (got %g)", (double)max_weight);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 && ((uintptr_t)tsdf & 3u) == 0 &&
                    ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)color & 3u) == 0 &&
                    (image_layout == 1 || ((uintptr_t)image & 3u) == 0),
                "tsdf_color_integrate: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 15u) == 0, "tsdf_color_integrate: workspace is not 16-byte aligned");
    // the volume is read and written while the inputs and the workspace are read: nothing written may overlap anything
    const size_t count = (size_t)batch * h * w, voxels = (size_t)nx * ny * nz;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4},
                                                          {valid, count},
                                                          {confidence, count * 4},
                                                          {image, count * (image_layout == 1 ? 3 : 12)}},
                                                  out[] = {{tsdf, voxels * 4},
                                                           {weight, voxels * 4},
                                                           {color, voxels * 12},
                                                           {workspace, need}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return a && b && x < y + bbytes && y < x + abytes;
    };
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "tsdf_color_integrate: the volume or the workspace aliases an input");
        for (int j = i + 1; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_color_integrate: tsdf, weight, color and the workspace alias one another");
    }
    ReprojectArgs r;
    for (int k = 0; k < 16; ++k) {
        r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(r.matrix[k]), "tsdf_color_integrate: non-finite matrix");
    }
    r.min_confidence = min_confidence;
    r.first = 0;
    for (size_t k = 0; k < 12 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(transforms[k]), "tsdf_color_integrate: non-finite transform");
    TsdfIntegrateArgs a = {};   // (A and b: per entry, from `transforms`)
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "tsdf_color_integrate: non-finite camera");
    }
    a.truncation = truncation;
    a.max_weight = max_weight;
    return launch_tsdf_color_integrate(r, a, transforms, weight_by_confidence, disparity, valid, confidence, image,
                                       image_layout, tsdf, weight, color, nx, ny, nz, batch, h, w, workspace,
                                       (hipStream_t)stream);
}

int pds_tsdf_color_gather_fwd(const int* index, const int* offsets, int edges_per_voxel, const float* tsdf,
                              const float* color, float* colors, long long capacity, int nx, int ny, int nz,
                              pds_stream_t stream) {
    PDS_REQUIRE(index && offsets && tsdf && color && colors, "tsdf_color_gather: null pointer");
    if (!tsdf_volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(edges_per_voxel == 3 || edges_per_voxel == 7,
                "tsdf_color_gather: edges_per_voxel must be 3 (extract) or 7 (mesh), got %d", edges_per_voxel);
    const size_t voxels = (size_t)nx * ny * nz;
    PDS_REQUIRE(voxels <= 0x7fffffffu / (unsigned)edges_per_voxel,
                "tsdf_color_gather: %d * nx * ny * nz does not fit 32-bit indices (%d, %d, %d)", edges_per_voxel, nx, ny,
                nz);
    PDS_REQUIRE(capacity >= 0, "tsdf_color_gather: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(((uintptr_t)index & 3u) == 0 && ((uintptr_t)offsets & 3u) == 0 && ((uintptr_t)tsdf & 3u) == 0 &&
                    ((uintptr_t)color & 3u) == 0 && ((uintptr_t)colors & 3u) == 0,
                "tsdf_color_gather: a 32-bit buffer is not 4-byte aligned");
    // the rows are read while colours are written
    const size_t rows = (size_t)capacity;
    const struct { const void* p; size_t bytes; } in[] = {{index, rows * 4}, {offsets, 8}, {tsdf, voxels * 4},
                                                          {color, voxels * 12}};
    const auto overlap = [](const void* a, size_t abytes, const void* b, size_t bbytes) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return abytes && bbytes && x < y + bbytes && y < x + abytes;
    };
    for (int j = 0; j < 4; ++j)
        PDS_REQUIRE(!overlap(colors, rows * 12, in[j].p, in[j].bytes), "tsdf_color_gather: the output aliases an input");
    return launch_tsdf_color_gather(index, offsets, edges_per_voxel, tsdf, color, colors, capacity, nx, ny, nz,
                                    (hipStream_t)stream);
}

int pds_tsdf_color_render_fwd(const float* weight, const float* color, int nx, int ny, int nz, const float* rays,
                              const float* camera, float min_weight, const float* depth, float* colors, int batch,
                              int h, int w, pds_stream_t stream) {
    PDS_REQUIRE(weight && color && rays && camera && depth && colors, "tsdf_color_render: null pointer");
    if (!tsdf_volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(batch > 0, "tsdf_color_render: bad batch %d", batch);
    PDS_REQUIRE(h > 0 && w > 0, "tsdf_color_render: bad shape (%d, %d)", h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu,
                "tsdf_color_render: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
    PDS_REQUIRE(!std::isnan(min_weight), "tsdf_color_render: min_weight is NaN");
    TsdfRaycastArgs a = {};
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "tsdf_color_render: non-finite camera");
    }
    PDS_REQUIRE(a.camera[0] > 0.f && a.camera[1] > 0.f, "tsdf_color_render: focal lengths must be positive (got %g, %g)",
                (double)a.camera[0], (double)a.camera[1]);
    for (size_t k = 0; k < 12 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(rays[k]), "tsdf_color_render: non-finite ray");
    PDS_REQUIRE(((uintptr_t)weight & 3u) == 0 && ((uintptr_t)color & 3u) == 0 && ((uintptr_t)depth & 3u) == 0 &&
                    ((uintptr_t)colors & 3u) == 0,
                "tsdf_color_render: a 32-bit buffer is not 4-byte aligned");
    // the volume and the depth are read while the colours are written
    const size_t voxels = (size_t)nx * ny * nz, count = (size_t)batch * h * w;
    const struct { const void* p; size_t bytes; } in[] = {{weight, voxels * 4}, {color, voxels * 12}, {depth, count * 4}};
    const auto overlap = [](const void* x, size_t xbytes, const void* y, size_t ybytes) {
        const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
        return p < q + ybytes && q < p + xbytes;
    };
    for (int j = 0; j < 3; ++j)
        PDS_REQUIRE(!overlap(colors, count * 12, in[j].p, in[j].bytes), "tsdf_color_render: the output aliases an input");
    a.min_weight = min_weight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.h = h;
    a.w = w;
    a.tiles_x = (w + kTsdfRaycastTile - 1) / kTsdfRaycastTile;
    a.tiles_y = (h + kTsdfRaycastTile - 1) / kTsdfRaycastTile;
    return launch_tsdf_color_render(a, rays, weight, color, depth, colors, batch, (hipStream_t)stream);
}

// (shared by the query and the entry point; 0: refused, the message is set)
static size_t icp_checked_bytes(int batch, int h, int w) {
    if (!(batch > 0 && h > 0 && w > 0)) {
        set_error(-1, "icp: bad shape (%d, %d, %d)", batch, h, w);
        return 0;
    }
    if ((size_t)batch * h * w > 0x7fffffffu) {
        set_error(-1, "icp: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
        return 0;
    }
    return icp_workspace_bytes(batch, h, w);
}

size_t pds_icp_workspace_bytes(int batch, int h, int w) { return icp_checked_bytes(batch, h, w); }

// (shared by pds_icp_system_fwd and pds_icp_system_robust_fwd; huber is read with robust only)
static int icp_system_entry(const float* disparity, const unsigned char* valid, const float* confidence,
                            float min_confidence, const float* matrix, const float* normals, const float* model_depth,
                            const float* model_normals, int model_batch, int hm, int wm, const float* camera,
                            const float* transforms, float max_distance, float min_cosine, double* system, float* rows,
                            int batch, int h, int w, void* workspace, size_t workspace_bytes, pds_stream_t stream,
                            bool robust, float huber) {
    PDS_REQUIRE(disparity && matrix && model_depth && model_normals && camera && transforms && system && workspace,
                "icp: null pointer");
    PDS_REQUIRE(!robust || huber > 0.f, "icp: huber must be positive (got %g)", (double)huber);
    const size_t need = icp_checked_bytes(batch, h, w);
    if (need == 0) return -1;
    PDS_REQUIRE(model_batch == 1 || model_batch == batch, "icp: model_batch must be 1 or batch = %d (got %d)", batch,
                model_batch);
    PDS_REQUIRE(hm > 0 && wm > 0 && hm < (1 << 24) && wm < (1 << 24), "icp: bad model shape (%d, %d)", hm, wm);
    PDS_REQUIRE((size_t)model_batch * hm * wm <= 0x7fffffffu,
                "icp: model_batch * hm * wm = %zu does not fit 32-bit indices", (size_t)model_batch * hm * wm);
    PDS_REQUIRE(workspace_bytes >= need, "icp: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!std::isnan(min_confidence), "icp: min_confidence is NaN");
    PDS_REQUIRE(max_distance > 0.f && std::isfinite(max_distance), "icp: max_distance must be positive and finite (got %g)",
                (double)max_distance);
    PDS_REQUIRE(!std::isnan(min_cosine), "icp: min_cosine is NaN");
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 && ((uintptr_t)normals & 3u) == 0 &&
                    ((uintptr_t)model_depth & 3u) == 0 && ((uintptr_t)model_normals & 3u) == 0 &&
                    ((uintptr_t)system & 3u) == 0 && ((uintptr_t)rows & 3u) == 0,
                "icp: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 7u) == 0, "icp: workspace is not 8-byte aligned");
    // the frame and the model are read while the partials, the system and the rows are written
    const size_t count = (size_t)batch * h * w, model = (size_t)model_batch * hm * wm;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {valid, count}, {confidence, count * 4},
                                                          {normals, count * 12}, {model_depth, model * 4},
                                                          {model_normals, model * 12}},
                                                  out[] = {{system, (size_t)batch * kIcpSystem * 8}, {rows, count * 28},
                                                           {workspace, need}};
    const auto overlap = [](const void* x, size_t xbytes, const void* y, size_t ybytes) {
        const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
        return x && y && p < q + ybytes && q < p + xbytes;
    };
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 6; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "icp: an output aliases an input");
        for (int j = i + 1; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes), "icp: an output aliases another output");
    }
    IcpArgs a = {};
    for (int k = 0; k < 16; ++k) {
        a.r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.r.matrix[k]), "icp: non-finite matrix");
    }
    a.r.min_confidence = min_confidence;
    a.r.first = 0;
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "icp: non-finite camera");
    }
    PDS_REQUIRE(a.camera[0] > 0.f && a.camera[1] > 0.f, "icp: focal lengths must be positive (got %g, %g)",
                (double)a.camera[0], (double)a.camera[1]);
    for (size_t k = 0; k < 12 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(transforms[k]), "icp: non-finite transform");
    a.max_distance = max_distance;
    a.min_cosine = min_cosine;
    a.h = h;
    a.w = w;
    a.hm = hm;
    a.wm = wm;
    a.model_batch = model_batch;
    a.tiles = icp_tiles(h, w);
    return launch_icp_system(a, transforms, disparity, valid, confidence, normals, model_depth, model_normals, system,
                             rows, batch, workspace, (hipStream_t)stream, robust, huber);
}

int pds_icp_system_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                       float min_confidence, const float* matrix, const float* normals, const float* model_depth,
                       const float* model_normals, int model_batch, int hm, int wm, const float* camera,
                       const float* transforms, float max_distance, float min_cosine, double* system, float* rows,
                       int batch, int h, int w, void* workspace, size_t workspace_bytes, pds_stream_t stream) {
    return icp_system_entry(disparity, valid, confidence, min_confidence, matrix, normals, model_depth, model_normals,
                            model_batch, hm, wm, camera, transforms, max_distance, min_cosine, system, rows, batch, h, w,
                            workspace, workspace_bytes, stream, false, 0.f);
}

int pds_icp_system_robust_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                              float min_confidence, const float* matrix, const float* normals, const float* model_depth,
                              const float* model_normals, int model_batch, int hm, int wm, const float* camera,
                              const float* transforms, float max_distance, float min_cosine, float huber, double* system,
                              float* rows, int batch, int h, int w, void* workspace, size_t workspace_bytes,
                              pds_stream_t stream) {
    return icp_system_entry(disparity, valid, confidence, min_confidence, matrix, normals, model_depth, model_normals,
                            model_batch, hm, wm, camera, transforms, max_distance, min_cosine, system, rows, batch, h, w,
                            workspace, workspace_bytes, stream, true, huber);
}

int pds_disparity_pyramid_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                              float min_confidence, float max_difference, float* const* out, int levels,
                              int source_level, int batch, int h, int w, pds_stream_t stream) {
    PDS_REQUIRE(disparity && out, "disparity_pyramid: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0, "disparity_pyramid: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu, "disparity_pyramid: batch * h * w = %zu does not fit 32-bit indices",
                (size_t)batch * h * w);
    PDS_REQUIRE(levels >= 1 && levels <= kPyramidLevels, "disparity_pyramid: levels must be in 1 .. %d (got %d)",
                kPyramidLevels, levels);
    PDS_REQUIRE(source_level >= 0, "disparity_pyramid: source_level must be >= 0 (got %d)", source_level);
    PDS_REQUIRE((h >> levels) >= 1 && (w >> levels) >= 1, "disparity_pyramid: level %d of %d x %d is empty", levels, w, h);
    PDS_REQUIRE(!std::isnan(min_confidence), "disparity_pyramid: min_confidence is NaN");
    PDS_REQUIRE(max_difference >= 0.f && std::isfinite(max_difference),
                "disparity_pyramid: max_difference must be finite and >= 0 (got %g)", (double)max_difference);
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0,
                "disparity_pyramid: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(pyramid_groups(batch, h, w) > 0, "disparity_pyramid: the blocks do not fit one launch");
    // a workgroup reads its block of the source and writes its pixels of every level: nothing written may overlap
    // anything read or another output
    const size_t count = (size_t)batch * h * w;
    const auto overlap = [](const void* x, size_t xbytes, const void* y, size_t ybytes) {
        const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
        return x && y && p < q + ybytes && q < p + xbytes;
    };
    size_t bytes[kPyramidLevels];
    for (int k = 0; k < levels; ++k) {
        PDS_REQUIRE(out[k], "disparity_pyramid: null pointer");
        PDS_REQUIRE(((uintptr_t)out[k] & 3u) == 0, "disparity_pyramid: a 32-bit buffer is not 4-byte aligned");
        bytes[k] = (size_t)batch * (h >> (k + 1)) * (w >> (k + 1)) * 4;
        PDS_REQUIRE(!overlap(out[k], bytes[k], disparity, count * 4) &&
                        (source_level > 0 || (!overlap(out[k], bytes[k], valid, count) &&
                                              !overlap(out[k], bytes[k], confidence, count * 4))),
                    "disparity_pyramid: an output aliases an input");
        for (int j = 0; j < k; ++j)
            PDS_REQUIRE(!overlap(out[k], bytes[k], out[j], bytes[j]), "disparity_pyramid: an output aliases another output");
    }
    return launch_disparity_pyramid(disparity, valid, confidence, min_confidence, max_difference, out, levels,
                                    source_level, batch, h, w, (hipStream_t)stream);
}

size_t pds_subpixel_cross_entropy_workspace_bytes(int n, int h, int w) {
    return sce_partial_doubles((size_t)n * h * w) * sizeof(double) + 256;
}

int pds_subpixel_cross_entropy_fwd(const float* similarities, const float* ground_truth, const float* weights,
                                   float* loss, float* lse, float* stats, int n, int planes, int h, int w,
                                   float diversity, int disparity_step, void* workspace, size_t workspace_bytes,
                                   pds_stream_t stream) {
    PDS_REQUIRE(similarities && ground_truth && loss && lse && stats && workspace, "subpixel_cross_entropy: null pointer");
    PDS_REQUIRE(n > 0 && planes > 0 && h > 0 && w > 0, "subpixel_cross_entropy: bad shape");
    PDS_REQUIRE(diversity > 0.f && disparity_step >= 1, "subpixel_cross_entropy: bad diversity / step");
    PDS_REQUIRE(workspace_bytes >= pds_subpixel_cross_entropy_workspace_bytes(n, h, w),
                "subpixel_cross_entropy: workspace too small");
    return launch_sce_fwd(similarities, ground_truth, weights, loss, lse, stats, (double*)workspace, n, planes, h, w,
                          diversity, disparity_step, (hipStream_t)stream);
}

int pds_subpixel_cross_entropy_bwd(const float* similarities, const float* ground_truth, const float* weights,
                                   const float* lse, const float* stats, const float* grad_loss,
                                   float* grad_similarities, int n, int planes, int h, int w, float diversity,
                                   int disparity_step, pds_stream_t stream) {
    PDS_REQUIRE(similarities && ground_truth && lse && stats && grad_loss && grad_similarities,
                "subpixel_cross_entropy_bwd: null pointer");
    PDS_REQUIRE(n > 0 && planes > 0 && h > 0 && w > 0, "subpixel_cross_entropy_bwd: bad shape");
    return launch_sce_bwd(similarities, ground_truth, weights, lse, stats, grad_loss, grad_similarities, n, planes, h,
                          w, diversity, disparity_step, (hipStream_t)stream);
}

int pds_subpixel_cross_entropy_weights_bwd(const float* similarities, const float* ground_truth, const float* lse,
                                           const float* stats, const float* grad_loss, float* grad_weights, int n,
                                           int planes, int h, int w, float diversity, int disparity_step,
                                           pds_stream_t stream) {
    PDS_REQUIRE(similarities && ground_truth && lse && stats && grad_loss && grad_weights,
                "subpixel_cross_entropy_weights_bwd: null pointer");
    PDS_REQUIRE(n > 0 && planes > 0 && h > 0 && w > 0, "subpixel_cross_entropy_weights_bwd: bad shape");
    return launch_sce_weights_bwd(similarities, ground_truth, lse, stats, grad_loss, grad_weights, n, planes, h, w,
                                  diversity, disparity_step, (hipStream_t)stream);
}

int pds_shift_concat_bwd(const float* grad_out, float* grad_left, float* grad_right, int batch, int channels, int h,
                         int w, int d_begin, int d_count, pds_stream_t stream) {
    PDS_REQUIRE(grad_out && grad_left && grad_right, "shift_concat_bwd: null pointer");
    PDS_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0 && d_begin >= 0 && d_count > 0,
                "shift_concat_bwd: bad shape");
    return launch_shift_concat_bwd(grad_out, grad_left, grad_right, batch, channels, h, w, d_begin, d_count,
                                   (hipStream_t)stream);
}

}  // extern "C"
