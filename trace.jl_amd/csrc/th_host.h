// th_host.h — what the translation units of libtracehip.so (csrc/tu_*.hip, each compiled on its own and linked into the one shared object) share on the host side: the
// context and scene objects behind the opaque handles of include/tracehip.h, error / buffer helpers, the frame scaffold, and the functions one unit calls in another.
// Three pieces carry the host's bookkeeping.  th_owned.h: DevBuf, OwnedEvent, OwnedStream and Pipe free what they hold and cannot be copied — ownership is decided THERE, by
// which object a member is declared in: trhip_ctx, trhip_scene, SceneGeometry and trhip_env are torn down by `delete`, a function's temporaries by its end, and nothing here
// keeps a list of buffers.  th_options.h: the options, one table row each, behind ctx->opt.  LastRecords below: what Lbuf holds after the last frame, written as a whole.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "th_options.h"  // (and include/tracehip.h)
#include "th_owned.h"
#include "th_bvh.h"
#include "th_kernels.h"
#include "th_trace2.h"
#include "th_trace8.h"  // (FallbackList, the 8-wide view's types: the kernels themselves are only instantiated by an EXPERIMENTS build)
#ifdef TRHIP_EXPERIMENTS
#include "th_trace4.h"
#include "th_trace7.h"
#endif
#include "th_trace3c.h"
#include "th_comm.h"

using namespace th;

// ---- context ------------------------------------------------------------------------------------------------------------------
extern thread_local std::string g_init_error;  // tu_api.hip: the message of a failed trhip_init

// What Lbuf holds after the last frame (trhip_last_sample_radiance, trhip_last_sample_stats).  A function that writes Lbuf sets `ctx->last = LastRecords{}` ("no records")
// after its refusals and before it first grows Lbuf, and assigns the whole struct once its stream has been synchronised: a frame that fails in between leaves no records.
struct LastRecords {
    uint64_t count = 0;  // float4 entries valid in Lbuf
    uint32_t layout = 0, npix = 1, spp = 1;  // how they are laid out (th_kernels.h, film_index)
    uint32_t kind = 0;  // whose they are: 1 a one-band path frame or trhip_film_accumulate's records (trhip_last_sample_stats reads them), 2 a map frame (exported through map_counts), 0 anything else
    enum Term : uint32_t { kNoTerm, kEnv, kEnvNee, kEmit } term = kNoTerm;  // which term's records are retained beside Lbuf's (docs/design/30-path-terms.md); the term writes it.
    // kEnv (tu_path_env.hip): Lbuf holds the folded records, env_base and env_rec what they were folded from (ctx->env_keep says how).  kEnvNee (tu_path_nee.hip): the same
    // records for trhip_last_escapes, but no relight — the base holds the map's light.  kEmit (tu_path_emit.hip): Lbuf holds L + Lh, emit_lh the emitted sums (trhip_last_emitted)
    bool env_records() const { return term == kEnv || term == kEnvNee; }
    void drop_env_records() {  // another render or an image pass between a path-env frame and its relight: the relight and trhip_last_escapes are refused after it
        if (env_records()) term = kNoTerm;
    }
};
// What trhip_path_env_relight needs of the path-env frame before it to run the film pass "exactly as the frame ran it" (valid while ctx->last.env_records()).
struct PathEnvKeep {
    DeviceSensor ds{};
    float filter_table[256] = {};
    uint32_t spp = 0, sample_offset = 0;
    uint64_t seed = 0, total_slots = 0, l_slots = 0;
    bool fused = false;
};
struct trhip_ctx;
struct trhip_scene;
// The extra shadow-ray lane of a path term (the NEE rays, the emitter rays; docs/design/30-path-terms.md): per pipe and parity of the depth a shadow queue (3 float4 arrays)
// with, for a term that asks for it, the reach of every entry (4 B); per pipe the NeeCounters (th_path_nee.h), zeroed per batch; one note byte per slot, whose meaning is the
// term's.  In tu_path_nee.hip.
struct ShadowLane {
    DevBuf sq[kMaxPipes][2][3], reach[kMaxPipes][2], ctr[kMaxPipes], note;
    size_t held(bool with_reach) const;  // what a frame reuses of it, for fits_in_hbm: the notes, the queues and, with_reach, the reaches
    int grow(trhip_ctx* ctx, int n_pipes, uint64_t queue_entries, uint64_t l_slots, bool with_reach);
    ShadowQueue queue(int pipe, int depth) const { return ShadowQueue{(float4*)sq[pipe][depth & 1][0].p, (float4*)sq[pipe][depth & 1][1].p, (float4*)sq[pipe][depth & 1][2].p}; }
    uint32_t* emitted(int pipe, int depth) const;  // NeeCounters::n of that depth: where the term's kernel counts the rays it appends
    int begin_batch(trhip_ctx* ctx, hipStream_t st, int pipe);
    // the any-hit launch over the lane's rays of `depth` (with_reach: each up to its reach): open rays add their contribution to L
    void launch_any(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, float4* L, int pipe, bool with_reach, Counters* ctr, void* overflow_slab);
};

struct Timer;
// Members are destroyed last to first: the workspace, then the pipes, then the two streams (trhip_shutdown, tu_api.hip).
struct trhip_ctx {
    int device = 0;
    Timer* active_timer = nullptr;  // the Timer of the render call in progress (hybrid launches mark the hand-over between their two walks in it)
    OwnedStream stream;
    OwnedStream stream2;  // shadow rays of depth d overlap with the closest-hit rays of depth d+1
    std::string err;
    int num_cu = 256;
    Options opt;  // trhip_set_option (th_options.h)
    LastRecords last;
    double bvh_device_ms = 0.0;  // device time of the last bvh_builder 3 build
    bool warned_idle_accelerator = false;  // (tu_path.hip: the one-time stderr note)
    bool warned_fallback_cliff = false;    // … and the one about a frame whose certified walk handed back more than a fifth of its rays
    double last_fallback_share = 0.0;      // fallback rays / closest-hit rays of the last frame that reported statistics (trhip_accelerator_note)
    Pipe pipes[kMaxPipes];
    // workspace (grown on demand, reused across calls)
    DevBuf q[2][3], sq[3], hits, Lbuf, pfilm, counters, sensor, table, film, scratch[4], overflow, wh_L, wh_parent, wh_coef, wh_pdf, wh_flags, occl, film_Lt, surv_list, surv_counts;
    // SPPM state (th_sppm.h): per film pixel, kept after trhip_render_sppm for trhip_sppm_state
    DevBuf sp_vp[7], sp_Ld, sp_tau, sp_radius, sp_N, sp_phi, sp_M, sp_counts, sp_starts, sp_entries, sp_grid, sp_ldist, sp_snap_M, sp_snap_phi, sp_snap_p, sp_snap_beta;
    DevBuf sp_terms, sp_rec[3], sp_rec_valid, sp_raysnap;  // sp_raysnap: {closest_total, shadow_total} after every batch's camera pass and photon pass
    uint32_t sp_pixels = 0;
    int64_t sp_photons = 0;
    // streaming wavefront (render_stream_impl)
    DevBuf st_terms, st_tags[2], st_frozen, st_counts, st_list[2][2][7];  // [closest|any][ping-pong][o, d, b, trav, st, depth, stack]
    DevBuf film_side;  // packed film pass: counter + the full descriptors of the samples whose range does not fit 30 bits (th_kernels.h, FilmSideTable)
    DevBuf poison;  // one byte per camera sample of the band: ShadeStream::poison
    DevBuf cert_cold;  // k_trace3c's CertCold (th_trace3c.h)
    DevBuf aov_rec;    // trhip_render_aov: the frame's per-sample records (th_aov.h, 80 B per camera sample)
    DevBuf ao_tmax;    // trhip_render_ao: the reach of every occlusion ray, beside the any-hit queue sq (th_ao.h, 4 B per queue entry)
    // dn_in, tp_in, up_in, dp_in: where the host entry points of the image-space passes stage their images, laid out by ImageStaging (th_image_pass.h) in the order a pass declares them
    DevBuf dn_work, dn_in;  // trhip_denoise: guides, two colour buffers and the base colour (th_denoise.h, 80 B per pixel); the host entry point's copy of film and planes
    DevBuf tp_in;           // trhip_temporal's host entry point: its copy of film, planes, history and the new history (th_temporal.h, 160 B per pixel); trhip_temporal_clip's: the same and
                            // the result's film (176 B); trhip_temporal_clip_device's film for a result that aliases its input (16 B); trhip_temporal_moments likewise (196 B; 16 B);
                            // trhip_temporal_motion's: trhip_temporal's and the id plane, the body matrices and the body table (176 B per pixel, 48 per body, 4 per primitive);
                            // trhip_temporal_clip_motion's: the same and the result's film (192 B per pixel); its _device variant's film for a result that aliases its input (16 B);
                            // trhip_temporal_split's: trhip_temporal_motion's and the direct film (192 B per pixel); trhip_film_add's two films (32 B per pixel)
    DevBuf up_in;      // trhip_upscale's host entry point: its copies of the five images (th_upscale.h; 64 B per low pixel, 65 per full-size pixel);
                       // trhip_temporal_upsample's likewise (th_temporal_upsample.h; 64 B per low pixel, 161 per full-size pixel); trhip_temporal_upsample_motion's: the same and
                       // the id plane, the body matrices and the body table (177 B per full-size pixel, 48 per body, 4 per primitive)
    DevBuf dp_work, dp_in;  // trhip_display: the 1 KiB metering histogram and a 16-byte state slot (th_display.h); the host entry point's copy of the film and its bytes (20 B per pixel)
    // adaptive sampling (th_adaptive.h): the last map frame's counts (kept for trhip_last_sample_radiance), their exclusive sum, the job list, hipcub's workspace, the
    // word k_map_reduce / k_sample_map sum into; the host entry points' copies of (m, v) and of the counts they return
    DevBuf map_counts, map_offsets, map_jobs, map_tmp, map_word, map_mv, map_out;
    // the path terms (docs/design/30-path-terms.md).  env_base: the path's own radiance records of a frame with a term (16 B per slot); Lbuf holds the term's fold.  env_rec: the
    // escape records of a path-env frame, with or without next-event estimation (32 B per slot).  emit_lh: an emit frame's per-sample emitted sums Lh (16 B per slot).
    // lane: the NEE rays' or the emitter rays' queues, counters and note bytes ("the vertex before was non-specular"; in an emit frame "… was specular")
    DevBuf env_base, env_rec, emit_lh;
    PathEnvKeep env_keep;
    ShadowLane lane;
    DevBuf cb_rc;     // one word: a host callback's return code, max-reduced over the ranks of a job (tu_sppm.hip)
    DevBuf ov8[2], fb_list[2], fb_counts[2];  // k_trace8: global stack levels, fallback lists + their counters / work cursors ([closest | any])
    Comm comm;  // multi-GPU job this context belongs to (trhip_comm_init); n_ranks == 1 without one; trhip_shutdown destroys its communicator before the context goes
};
static_assert(!std::is_copy_constructible_v<trhip_ctx>, "trhip_ctx owns its streams, pipes and workspace");

struct HostPrim {
    uint32_t kind;       // 0 triangle, 1 sphere
    float v[9];          // triangle vertices (world)
    float n[9];          // vertex normals
    uint32_t meta;       // material | flags
    uint32_t sphere_id;  // for spheres
};

// What a commit derives from the primitives alone: the host records, both trees and every device buffer made from them.  A scene holds it through a shared_ptr: its relit
// views (trhip_scene_relight) share it, each with its own lights.  The device buffers go with the last handle that holds them.
struct SceneGeometry {
    uint64_t id = 0;  // trhip_scene_geometry_id: a new value for every tree this geometry is committed with (0 = never committed)
    int max_node_primitives = -1;  // what the last trhip_scene_commit built the trees with (-1: a caller's tree alone, trhip_scene_set_bvh)
    std::vector<MaterialRec> materials;
    std::vector<float> base_colour;  // 4 floats per material: its base colour (include/tracehip.h, trhip_aov_sample) and a zero
    std::vector<HostPrim> prims;  // caller order
    // the two optional mesh arrays (shapes/triangle_mesh.jl:11-14), beside the primitives and only when some mesh carries them (no scene of the reference does):
    // prim_tan[9 i ..] = primitive i's vertex tangents (PRIM_HAS_TANGENTS), prim_uv[7 i ..] = its corner (u, v)s and a "has" flag; empty = none
    std::vector<float> prim_tan, prim_uv;
    std::vector<SphereRec> spheres;
    std::vector<HostAABB> sphere_bounds;
    FlatBVH bvh;
    // ---- hybrid mode (th_trace3c.h): `bvh` above is the CANONICAL tree (the reference's construction, or the host's own tree) — slots, shading records, the inspection API
    // and the answers are its; `acc` is the library's tree over the same primitives, which most rays walk instead
    FlatBVH acc;  // order[k] = caller primitive of accelerator slot k; empty without an accelerator
    // the any-hit pre-pass candidates (th_trace2.h, k_any_occluders): the largest triangles' ordered slots by area and their leaves' boxes; the light stage orders them
    std::vector<uint32_t> occ_slots;
    std::vector<float> occ_boxes;
    DevBuf d_leaf_boxes;  // one-leaf scenes: the boxes of the leaf's triangles in slot order (th_leaf2.h)
    DevBuf d_nodes, d_prims, d_nrm, d_tan, d_shade, d_spheres, d_materials, d_base_colour, d_wnodes, d_w8nodes, d_w8tris;
    DevBuf d_shade_cold;  // one ShadeCold (th_scene.h): the sphere, material and tangent pointers k_shade_path reads outside its matte path
    DevBuf d_acc_w4nodes;  // the accelerator four children wide (th_trace3c4.h)
    DevBuf d_acc_wnodes, d_acc_prims, d_slot_boxes, d_sphere_boxes, d_sphere_slots, d_sphere_cert;
};
static_assert(!std::is_copy_constructible_v<SceneGeometry>, "SceneGeometry owns its device buffers");

// The views of a committed geometry: pointers into its buffers (the light pointers and orders patched in by the light stage) and what the commit found out about it.  Plain
// values that own nothing: a relit view copies its base's (tu_scene.hip, trhip_scene_relight).
struct SceneViews {
    bool has_materialless_prim = false;  // set at commit: some GeometricPrimitive has no material (path and Whitted refuse such a scene; SPPM crosses it, th_sppm.h XING; the trace entry points accept it)
    DeviceScene dev{};
    WideScene wide{};
    Wide8Scene w8{};              // the 8-wide view of the triangles' subtree (th_wide8.h / th_trace8.h)
    uint32_t w8_nodes = 0, w8_depth = 0;
    bool partial_spheres = false;  // some sphere is clipped (z range or ϕ_max): traversal kernels with the general sphere test
    bool wide_ok = false;
    bool w8_ok = false;            // the 8-wide view exists (th_trace8.h)
    bool literal_only = false;     // a caller-supplied BVH whose boxes do not nest (trhip_scene_set_bvh): literal kernels only
    bool hybrid_ok = false;        // the accelerator exists and its leaves carry the canonical leaves' boxes bit for bit
    std::string bvh_note;          // why a default commit ended with one tree (trhip_scene_bvh_note)
    int bvh_mode = 0;              // what trhip_scene_commit / trhip_scene_set_bvh built: 0 the library's tree alone, 1 the canonical (reference / host) tree alone, 2 both
    WideScene wide_acc{};
    DeviceScene dev_acc{};         // dev with the accelerator's primitive records
    CertScene cert{};
};
// A scene handle: the geometry it shares, the views above, and what the light stage (tu_scene.hip, commit_lights) owns — the lights, the light records and the any-hit test
// orders computed from them.  It cannot be copied, so a relit view starts with the light stage's members default-constructed whatever is added to them.
struct trhip_scene : SceneViews {
    trhip_ctx* ctx = nullptr;
    std::shared_ptr<SceneGeometry> g = std::make_shared<SceneGeometry>();
    bool relit = false;  // a relit view (trhip_scene_relight): its geometry is fixed, a commit runs the light stage alone
    std::vector<LightRec> lights;
    bool committed = false;
    DevBuf d_lights, d_leaf_order, d_acc_leaf_order, d_occ_slots, d_occ_boxes;
    uint32_t n_occluders = 0;     // the scene's largest triangles, tested first by any-hit rays (th_trace2.h, k_any_occluders)
};
static_assert(!std::is_copy_constructible_v<trhip_scene>, "trhip_scene owns the light stage's buffers");

// some light is a DirectionalLight (kind 2): the shading kernels run their DIRL variants (th_device.h, sample_li)
inline bool has_directional_light(const trhip_scene* s) {
    for (const LightRec& l : s->lights)
        if (l.kind == 2) return true;
    return false;
}

inline int fail(trhip_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_init_error = buf;
    return code;
}
#define HIP_TRY(ctx, expr)                                                                                       \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return fail(ctx, TRHIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define NCCL_TRY(ctx, expr)                                                                                                  \
    do {                                                                                                                     \
        ncclResult_t r_ = (expr);                                                                                            \
        if (r_ != ncclSuccess) return fail(ctx, TRHIP_ERR_HIP, "%s failed: %s", #expr, rccl_api()->GetErrorString ? rccl_api()->GetErrorString(r_) : "RCCL error"); \
    } while (0)

inline int ensure(trhip_ctx* ctx, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return 0;
    HIP_TRY(ctx, b.reset());
    if (bytes == 0) bytes = 16;
    HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return 0;
}
inline void release(DevBuf& b) { (void)b.reset(); }  // for the places that free early on purpose; everything else goes with its owner
inline int upload(trhip_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {
    if (int rc = ensure(ctx, b, bytes)) return rc;
    if (bytes) HIP_TRY(ctx, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
// a staging array that is NOT zero-filled on allocation (std::vector value-initialises: 1.5 GB of single-threaded memset for a 10 M-triangle scene's records, all of which the
// fill loops overwrite)
template <class T>
struct RawArray {
    std::unique_ptr<T[]> p;
    size_t n = 0;
    explicit RawArray(size_t count) : p(new T[count ? count : 1]), n(count) {}
    T* data() { return p.get(); }
    const T* data() const { return p.get(); }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};
// f(begin, end) over [0, n) on the host's cores (scene commit's loops over millions of nodes / primitives); ranges are disjoint and contiguous
template <class F>
inline void parallel_for(size_t n, F&& f, size_t grain = size_t(1) << 15) {
    const size_t want = n / std::max<size_t>(1, grain);
    const size_t nt = std::min<size_t>({want, (size_t)std::max(1u, std::thread::hardware_concurrency()), (size_t)32});
    if (nt <= 1) {
        f((size_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(nt - 1);
    const size_t step = (n + nt - 1) / nt;
    for (size_t t = 1; t < nt; ++t) th.emplace_back([&f, t, step, n] { f(std::min(n, t * step), std::min(n, (t + 1) * step)); });
    f((size_t)0, std::min(n, step));
    for (auto& x : th) x.join();
}
// do camera rays start far outside the scene (more than 4 scene extents away)?  Then the hybrid walk's launch over them takes the per-axis form of its cull bound
// (TraceOut::far_hint, th_trace3c.h): the scalar margin scales with the reach D of the rays' arithmetic, which is what such a distance inflates
inline bool far_camera(const trhip_scene* sc, const trhip_sensor* sn) {
    if (!sc->hybrid_ok || !sn) return false;
    const float* rb = sc->wide_acc.root_box;
    const float o[3] = {sn->camera_to_world[3], sn->camera_to_world[7], sn->camera_to_world[11]};
    float reach = 0.0f, extent = 0.0f;
    for (int a = 0; a < 3; ++a) {
        reach = std::fmax(reach, std::fmax(std::fabs(rb[a] - o[a]), std::fabs(rb[3 + a] - o[a])));
        extent = std::fmax(extent, rb[3 + a] - rb[a]);
    }
    return reach > 4.0f * extent;
}
inline int grid_for(const trhip_ctx* ctx, uint64_t n, int blocks_per_cu) {
    const uint64_t need = (n + kBlock - 1) / kBlock;
    const uint64_t cap = (uint64_t)ctx->num_cu * blocks_per_cu;
    return (int)std::max<uint64_t>(1, std::min(need, cap));
}

// TRHIP_FRAME_TIMING=1: host-side time between the stages of a render call, one line per stage on stderr
struct HostClock {
    bool on = std::getenv("TRHIP_FRAME_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void tick(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[frame] %-32s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - t).count());
        t = now;
    }
};
struct Timer {
    trhip_ctx* ctx;
    bool on;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[8];  // 0 raygen, 1 closest, 2 shade, 3 any, 4 film; 5-7: sub-classes of an integrator (tu_sppm.hip)
    std::vector<std::pair<size_t, hipEvent_t>> marks;       // hybrid mode: (index into ev[1], event between the certified walk and the fallback walk of that closest-hit launch)
    explicit Timer(trhip_ctx* c, bool enable) : ctx(c), on(enable) { c->active_timer = this; }
    ~Timer() {
        if (ctx->active_timer == this) ctx->active_timer = nullptr;
        for (auto& v : ev)
            for (auto& p : v) {
                (void)hipEventDestroy(p.first);
                (void)hipEventDestroy(p.second);
            }
        for (auto& m : marks) (void)hipEventDestroy(m.second);
    }
    void mark_fallback(hipStream_t st) {  // called by launch_trace between the two walks of a hybrid closest-hit launch (inside begin(1) .. end(1))
        if (!on || ev[1].empty()) return;
        hipEvent_t e;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, st);
        marks.push_back({ev[1].size() - 1, e});
    }
    double fallback_total(uint32_t* launches) {  // time from each mark to the end of its launch
        double ms = 0;
        for (auto& m : marks) {
            float t = 0;
            if (m.first < ev[1].size()) (void)hipEventElapsedTime(&t, m.second, ev[1][m.first].second);
            ms += t;
        }
        *launches = (uint32_t)marks.size();
        return ms;
    }
    void begin(int cls, hipStream_t st) {
        if (!on) return;
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, st);
        ev[cls].push_back({a, b});
    }
    void end(int cls, hipStream_t st) {
        if (!on) return;
        (void)hipEventRecord(ev[cls].back().second, st);
    }
    double total(int cls, uint32_t* launches) {
        double ms = 0;
        for (auto& p : ev[cls]) {
            float t = 0;
            (void)hipEventElapsedTime(&t, p.first, p.second);
            ms += t;
        }
        *launches = (uint32_t)ev[cls].size();
        return ms;
    }
};
// The event pair around the device work of one call (trhip_stats.ms_total).  Owned: whichever way the function returns, the events go with it.
struct FrameEvents {
    OwnedEvent e0, e1;
    hipError_t begin(hipStream_t st) {  // creates the pair and records its first event
        if (hipError_t e = e0.create_timed()) return e;
        if (hipError_t e = e1.create_timed()) return e;
        return hipEventRecord(e0, st);
    }
    hipError_t end(hipStream_t st) { return hipEventRecord(e1, st); }
    float ms() const {  // after the stream has been synchronised
        float t = 0;
        (void)hipEventElapsedTime(&t, e0, e1);
        return t;
    }
};
// ---- the frame scaffold of the render entry points ----------------------------------------------------------------------------------
// Physical queue layout: kSeg segments of this many entries (th_kernels.h "SegQueue").  A segment receives at most P / kSeg + O(kSegGran) entries per bounce by
// construction; `extra_segment_entries` is what an integrator appends to a segment on top of that (the streaming frame's resumed rays).
inline uint64_t queue_cap(uint64_t P, uint64_t extra_segment_entries = 0) {
    return ((P + kSeg - 1) / kSeg + 2 * kSegGran + extra_segment_entries + kSegGran - 1) / kSegGran * kSegGran;
}
// what the path frames' pipes hold of a frame's queues: reused by the next frame, so it counts as available to it
inline size_t held_in_pipes(const trhip_ctx* ctx) {
    size_t held = 0;
    for (auto& pp : ctx->pipes) {
        held += pp.hits.bytes;
        for (auto& a : pp.q)
            for (auto& b : a) held += b.bytes;
        for (auto& b : pp.sq) held += b.bytes;
    }
    return held;
}
// The streams and events of pipe `index` (th_owned.h): made on first use, and completed when an earlier call got only part of the way, so a frame never runs on a half-made
// pipe.  honour_priority: the second stream is made at the level option "stream2_priority" asks for — the classic path frame passes true, the streaming frame and SPPM
// false.  KNOWN, kept as it was: whichever of them runs first on a context makes the stream, so the first caller decides the shadow stream's priority for the context's life.
inline int ensure_pipe(trhip_ctx* ctx, int index, bool honour_priority) {
    Pipe& pp = ctx->pipes[index];
    // the shadow-ray stream gets its own priority level: streams of one level can share a hardware queue (then any(d) and
    // closest(d+1) run one after the other: measured in the first context of a process), streams of different levels cannot
    int prio_lo = 0, prio_hi = 0;
    if (honour_priority && !pp.st2 && ctx->opt.stream2_priority) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const int prio = ctx->opt.stream2_priority > 0 ? prio_hi : prio_lo;
    HIP_TRY(ctx, pp.complete(prio_hi != prio_lo ? &prio : nullptr));
    return 0;
}
// The one-batch entry points (aov, ao, and the image-space passes: denoise, denoise_var, temporal and temporal_clip, temporal_moments, upscale, display, temporal_upsample) refuse a frame that needs more than 0.9 of what is free plus what the context already holds for it (`held`, reused).
// *free_gb is that sum, for the caller's sentence.
inline int fits_in_hbm(trhip_ctx* ctx, double need, size_t held, bool* fits, double* free_gb) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    *fits = !(need > 0.9 * (double)(free_b + held));
    *free_gb = (double)(free_b + held) * 1e-9;
    return 0;
}
// Where a call writes an image: the caller's pointer when that is device memory, otherwise ctx->film grown to hold it, which copy_back brings to the caller.
inline int stage_output(trhip_ctx* ctx, void* out, bool out_is_device, size_t bytes, void** d) {
    *d = out;
    if (out_is_device) return 0;
    if (int rc = ensure(ctx, ctx->film, bytes)) return rc;
    *d = ctx->film.p;
    return 0;
}
inline int copy_back(trhip_ctx* ctx, void* out, bool out_is_device, const void* d, size_t bytes) {
    if (!out_is_device) HIP_TRY(ctx, hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ---- functions one unit calls in another ---------------------------------------------------------------------------------------------
// tu_scene.hip
int upload_scene(trhip_scene* s);
int upload_accelerator(trhip_scene* s);
// tu_lbvh.hip
int build_bvh_device(trhip_ctx* ctx, const std::vector<HostAABB>& pb, FlatBVH& out);
int build_bvh_device_sah(trhip_ctx* ctx, const std::vector<HostAABB>& pb, int max_node_prims, bool split_coincident, FlatBVH& out, double* ms_device);
// tu_trace.hip
int trace_grid(const trhip_ctx* ctx);
int ensure_overflow(trhip_ctx* ctx);
WideScene wide_view(const trhip_ctx* ctx, const trhip_scene* sc);
// The closest-hit kernel family a launch on this scene runs (closest_kernel: the ONE place that decides it — launch_trace and launch_trace3c branch on the answer, traversal_info and
// trhip_closest_kernel_name report it), and whether it takes its BIG variant (scenes larger than the last-level cache; the visit-counting kernels have none).  Trace3d, Trace4,
// Trace7 and Trace8 are kernels of the EXPERIMENTS build.
enum class ClosestKernel { Literal, Trace2, Leaf, Trace3, Trace3c, Trace3c4, LeafC, Trace3d, Trace4, Trace7, Trace8 };
struct ClosestChoice {
    ClosestKernel kernel;
    bool big;
};
ClosestChoice closest_kernel(const trhip_ctx* ctx, const trhip_scene* sc, bool cnt, bool indirect);
void traversal_info(const trhip_ctx* ctx, const trhip_scene* sc, uint32_t* trav, uint32_t* node_bytes);
void launch_trace(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, SegQueue q, const float4* ro, const float4* rd, const float* tmax, TraceOut out, uint32_t* work_cursors,
                  Counters* ctr, void* overflow_slab = nullptr);
void launch_trace2_stream(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, SegQueue q, const float4* ro, const float4* rd, TraceOut out, uint32_t* work_cursors, void* overflow_slab,
                          Counters* ctr, const StreamCtl& sx);
// tu_trace3.hip / tu_trace8.hip: the kernel families launch_trace picks from
void launch_trace3(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, bool cnt, bool full_only, bool big, const SegQueue& q, const float4* ro, const float4* rd, const float* tmax,
                   const TraceOut& out, uint32_t* work_cursors, uint2* ov, Counters* ctr, bool on_accelerator = false);
void launch_trace4(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, bool cnt, bool full_only, const SegQueue& q, const float4* ro, const float4* rd, const float* tmax,
                   const TraceOut& out, uint32_t* work_cursors, uint2* ov, Counters* ctr);
// tu_trace3c.hip: the hybrid mode's certified walks on the accelerator tree (th_trace3c.h)
bool hybrid_active(const trhip_ctx* ctx, const trhip_scene* sc);
const char* hybrid_idle_reason(const trhip_ctx* ctx, const trhip_scene* sc);
WideScene wide_view_acc(const trhip_ctx* ctx, const trhip_scene* sc);
void launch_trace3c(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, ClosestChoice pick, bool cnt, bool full_only, const SegQueue& q, const float4* ro, const float4* rd, const float* tmax,
                    const TraceOut& out, uint32_t* work_cursors, uint2* ov, Counters* ctr, const FallbackList& fb);
void launch_leaf_c(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, bool cnt, bool full_only, const SegQueue& q, const float4* ro, const float4* rd, const float* tmax,
                   const TraceOut& out, Counters* ctr, const FallbackList& fb);
void launch_trace7(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool cnt, bool full_only, bool big, const SegQueue& q, const float4* ro, const float4* rd, const float* tmax,
                   const TraceOut& out, uint32_t* work_cursors, uint2* ov, Counters* ctr, const FallbackList& fb);
void launch_trace8(trhip_ctx* ctx, hipStream_t st, const trhip_scene* sc, bool any, bool cnt, bool full_only, const Wide8Scene& w8, const SegQueue& q, const float4* ro, const float4* rd,
                   const float* tmax, const TraceOut& out, uint32_t* work_cursors, uint32_t* ov8, Counters* ctr, const FallbackList& fb);
// tu_path.hip
void derive_sensor(const trhip_sensor* sn, DeviceSensor& d);
// … the film pass: packed (both filter radii in (0, 1]) or wide.  A frame asks film_packed which pass it gets, gets the wide pass's film positions from
// ensure_film_samples and hands its records to launch_film.
// A map frame (trhip_render_path_map) has a per-pixel sample count instead of one spp: the records keep the dense max_spp layouts, the frame's camera samples are the job
// list (th_adaptive.h, k_map_expand) and the gather stops at counts[pix].
struct MapFrame {
    const uint32_t* counts;  // device: one per sample pixel
    const uint32_t* jobs;    // device: `total` dense sample-major slots
    uint64_t total;          // Σ counts
};
bool film_packed(const DeviceSensor& ds);
int ensure_film_samples(trhip_ctx* ctx, bool packed, uint64_t total_slots);
void launch_film(trhip_ctx* ctx, hipStream_t st, const DeviceSensor& ds, const DeviceSensor* dsp, const float4* L, uint64_t total_slots, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                 float4* d_film, bool fused, const MapFrame* map = nullptr);
// … the one place that turns device counters and event times into trhip_stats.  A frame's stats are: zeros, stats_add_counters for every Counters block it ran on,
// stats_fill_times, and what only the caller knows (camera_samples, n_batches, max_depth_reached, an integrator's ms_sub / count_sub)
void stats_add_counters(trhip_stats& s, const Counters& h);  // += the ray, node-visit and primitive-test totals, the fallback totals and the fallback reasons (count_sub)
void stats_fill_times(trhip_ctx* ctx, const trhip_scene* sc, Timer& tm, const FrameEvents& ev, trhip_stats& s);  // ms_total, Timer classes 0-4, the fallback share, traversal_info
void stats_accumulate(trhip_stats& sum, const trhip_stats& band);  // a banded frame: += every additive field; max_depth_reached, traversal, node_bytes as the last band has them
// tu_adaptive.hip: a map frame's job list from ctx->map_counts (npix counts, already on the device).  sum_on_device: Σ counts and "some count lies above max_spp" come from
// the device (8 bytes read back) into *total and *above; otherwise the caller has both.  Nothing is built when *above or *total == 0.
int map_job_list(trhip_ctx* ctx, uint32_t npix, uint32_t max_spp, bool sum_on_device, uint64_t* total, bool* above);
// A path term: what a frame adds to trhip_render_path's frame (docs/design/30-path-terms.md: the hooks, their order within a depth, how to add a term).  The classic
// wavefront's loop (tu_path.hip, render_impl_band) is handed one, the way it is handed a MapFrame, and asks it at these places, in this order.
struct PathTermShape {  // what the loop has planned by the time it asks for the buffers
    int n_pipes;
    uint64_t queue_entries, total_slots, l_slots;
    double film_bytes;  // what an unfused film pass reads per sample: buffers of its own beside the term's
    uint32_t spp;
};
struct PathTerm {
    float4* base = nullptr;  // l_slots records, set by buffers(): the shading kernels' and the shadow rays' target in Lbuf's place; Lbuf receives the fold
    virtual ~PathTerm() = default;
    virtual int check(trhip_ctx* ctx, const trhip_scene* scene) = 0;  // the term's refusals, after the path frame's own
    virtual int early_budget(trhip_ctx*, uint64_t /*total_slots*/, double /*film_bytes*/, uint32_t /*spp*/) { return 0; }  // a refusal before batch planning, before any pipe is grown
    virtual double slot_bytes() const = 0;             // batch planning: bytes per sample slot beside Lbuf …
    virtual double path_bytes() const { return 0.0; }  // … and per path in flight beside the loop's own 212
    virtual int buffers(trhip_ctx* ctx, const PathTermShape& s) = 0;  // the late budget refusal, then the buffers
    virtual int clear(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots) = 0;  // at the frame's start, after the loop's own clears
    virtual int begin_batch(trhip_ctx*, hipStream_t, int /*pipe*/) { return 0; }  // on the pipe's main stream, before raygen
    // after the closest-hit trace of `depth`, before its shade launch: every ray of the depth has its final answer
    virtual void after_closest(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth,
                               uint32_t hits_have_bary, int pipe) = 0;
    // directly after the point-light any-hit trace of `depth`, on its stream, with its Counters and its overflow slab
    virtual void after_any(trhip_ctx*, hipStream_t, const trhip_scene*, uint32_t /*cap*/, int /*depth*/, int /*pipe*/, Counters*, void* /*overflow_slab*/) {}
    virtual void fold(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots, float4* out) = 0;  // out = base and what the term adds; the film pass and trhip_last_sample_radiance read out
    virtual void retain(trhip_ctx* ctx, const PathEnvKeep& film_pass) = 0;  // after the frame's stream has been synchronised: ctx->last.term, and what a later call needs
};
// tu_path.hip: trhip_render_path's frame — its refusals in its order, the classic wavefront without bands — as a map frame and / or with a term
int render_path_frame(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, void* out, bool out_is_device,
                      trhip_stats* stats, const MapFrame* map, PathTerm* term);
// the parameter block of a term's entry point (scale, flags, reserved): checked before any handle is looked at, and none of it needs a device
template <class Params>
int path_params_check(trhip_ctx* ctx, const Params* prm, uint32_t known_flags, const char* entry) {
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "%s: scale must be finite and >= 0", entry);
    if (prm->flags & ~known_flags) return fail(ctx, TRHIP_ERR_INVALID, "%s: unknown flag bits 0x%x", entry, prm->flags & ~known_flags);
    for (uint32_t r : prm->reserved)
        if (r != 0) return fail(ctx, TRHIP_ERR_INVALID, "%s: reserved must be 0", entry);
    return 0;
}
// the tail of trhip_last_sample_radiance, trhip_last_escapes and trhip_last_emitted: `launch(dst)` exports ctx->last's records to scratch, which is brought to the caller
template <class Launch>
int read_back_records(trhip_ctx* ctx, float* out, uint64_t n_floats, Launch&& launch) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, ctx->scratch[0], n_floats * sizeof(float))) return rc;
    if (ctx->last.count) launch(ctx->scratch[0].p, dim3((unsigned)((ctx->last.count + 255) / 256)));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->scratch[0].p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
// tu_path_env.hip: the environment term (th_path_env.h; docs/design/26-path-env.md).  The term with next-event estimation (tu_path_nee.hip) is this one plus the lane: it
// keeps the checks, the clears, the records and the keep, and replaces the per-depth kernel and the fold.
struct trhip_env;
struct EnvTerm : PathTerm {
    const trhip_env* env;
    float scale;
    uint32_t flags;
    float4* rec = nullptr;  // 2 * l_slots: {beta.xyz, depth}, {dir.xyz, 0}
    EnvTerm(const trhip_env* e, float s, uint32_t f) : env(e), scale(s), flags(f) {}
    int check(trhip_ctx* ctx, const trhip_scene* scene) override;  // null, another context's, a scale that takes the largest texel to +Inf
    int early_budget(trhip_ctx* ctx, uint64_t total_slots, double film_bytes, uint32_t spp) override;
    double slot_bytes() const override { return 3.0 * sizeof(float4); }  // the base records and the escape records beside Lbuf
    int buffers(trhip_ctx* ctx, const PathTermShape& s) override;
    int clear(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots) override;
    void after_closest(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t hits_have_bary,
                       int pipe) override;
    void fold(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots, float4* out) override;
    void retain(trhip_ctx* ctx, const PathEnvKeep& film_pass) override;
    virtual LastRecords::Term kind() const { return LastRecords::kEnv; }
};
// tu_path_nee.hip: a material that mixes specular and non-specular lobes (the NEE term and the emit term refuse it)
int path_mixed_lobes_check(trhip_ctx* ctx, const trhip_scene* scene, const char* entry);
// tu_whitted.hip
int render_whitted_impl(trhip_ctx* ctx, const trhip_scene* scene, const DeviceSensor& ds, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                        void* d_film, trhip_stats* stats);
