// th_options.h — the options of a context (trhip_set_option): their fields with their defaults, ONE table that says for each name how a value is turned into its field
// and which values only the EXPERIMENTS build carries, and the one function that reads the table.  No HIP here: tests/host/options_main.cpp builds this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#pragma GCC visibility push(default)
#include "../../include/tracehip.h"
#pragma GCC visibility pop

constexpr int kMaxPipes = 8;

struct Options {
    bool count_visits = false;
    bool timing = true;
    uint64_t batch_paths = 0;  // 0 = as many whole sample passes as fit in free HBM (fewer launches, fewer traversal tails)
    int pipelines = 1;    // concurrent wavefront batches (each on its own stream pair); measured: no gain, every batch pays every tail
    uint32_t debug_trace_budget = 0;  // DIAGNOSTIC: k_trace2 abandons rays after this many node fetches (results wrong; measures bulk vs tail)
    int bvh_builder = -1;  // BVHAccel construction: 0 = binned SAH on the host (th_bvh.h), 1 = linear BVH on the device (th_lbvh.h), 3 = the host builder's
                           // binned SAH on the device (th_sahb.h: the same tree), 2 = the reference's own construction node for node (th_bvh_ref.h:
                           // the tree Trace.jl builds, hence its tie-breaks), -1 = automatic: builder 3 from 64 Ki primitives on, builder 0 below and
                           // for the scenes builder 3 hands back.  Measured (r3): building the tree 18 ms (1 M triangles) / 53 ms (10 M) on the device
                           // against ~0.17 s / ~1.5 s on the host, commit 0.39 -> 0.26 s and 3.67 -> 2.37 s; the LBVH builds a 25-35 % costlier tree
    bool occluder_pretest = true;    // any-hit rays test the scene's largest triangles before the walk (option "occluder_pretest")
    int stream2_priority = -1;       // shadow-ray stream: 1 highest priority, -1 lowest, 0 the default level (option "stream2_priority", read when the streams are created)
    bool leaf_kernel = true;         // one-leaf scenes run k_trace_leaf instead of k_trace2 (option "leaf_kernel", for A/B)
    int slab_margin_log2 = 14;       // k_trace2 / k_trace3 add the slab clauses the reference's box test lost, on boxes grown by 2^-this x the ray's reach
                                     // (th_trace2.h, slab_test2); 0 = the reference's loose test alone (its exact visit set)
    int band_tile_rows = 0;          // DIAGNOSTIC / tests: render frames in bands of this many tile rows (0 = one band unless the samples do not fit in HBM)
    uint32_t tiny_scene_prims = 16;  // scenes of at most this many primitives get a single-leaf BVH (th_bvh.h); 0 = always build the hierarchy
    bool film_relayout = true;  // packed film pass: gather from a pixel-group-major copy of the radiance records (k_film_pack_transpose) instead of the integrators' sample-major order
    int any_on_accelerator = -1;  // hybrid mode: any-hit rays without a zero direction component walk the library's tree (TraceOut::zero_mode): 1 always, 0 never, -1 where the
                                  // integrator asks for it (TraceOut::any_acc_hint: SPPM).  Option "any_on_accelerator"
    bool wide4 = true;  // hybrid mode: the accelerator is also laid out four children wide and the certified walk runs on that (th_trace3c4.h); option "wide4", read at commit and at launch
    bool leaf_queue = false;  // hybrid mode: the certified walk queues the leaves it reaches and tests them 64 at a time with whichever lanes (th_trace3d.h, option "leaf_queue")
    int node_layout = 0;  // children-in-parent nodes: 0 depth-first, 1 the two interior children of a node in one aligned 128-byte line (option "node_layout", read at commit; tu_scene.hip)
    bool overlap = true;   // shadow rays of depth d on a second stream beside the closest-hit rays of depth d+1 (option "overlap").  On again since round 5: with the four-wide
                           // certified walk no longer saturating VALU issue the shadow kernels fill its gaps and tails — 256 spp, off / on: S-mesh 325.5 / 314.5 ms, S-blob 234.8 / 222.3,
                           // S-cornell 160.4 / 157.1, 10.5 M triangles 376.4 / 367.7.  (Rounds 2-4 measured it neutral — S-cornell 158.2 / 157.9, S-mesh 399 / 393 — and kept it off.)
    int compose_spheres = -1;  // commit: spheres as a chain of leaves above the triangles' subtree, what k_trace8 needs of a scene with spheres
                               // (option "compose_spheres": 1 / 0 = one SAH tree over everything / -1 = when "traversal" is 4 at commit time)
    int traversal = 3;  // 1 = literal accel/bvh.jl loop, 2 = children-in-parent nodes + per-lane ray replacement, 3 = 2 with leaves postponed (while-while),
                        // 4 = 8-wide quantised nodes in the binary walk's order (th_trace8.h; scenes / rays it cannot take run 3), 6 = 3 with two rays per lane (th_trace4.h),
                        // 7 = closest-hit rays front to back with tie detection, flagged rays re-traced by 3 (th_trace7.h); any-hit rays as 3
    bool leaf_sorted = false;  // one-leaf scenes: rays grouped by the primitives they can hit before the leaf is walked (th_leaf2.h, option "leaf_sorted"); exact, measured SLOWER
                               // (S-cornell closest-hit 49.2 -> 60.2 ms, any-hit 15.9 -> 30.8: twelve candidate tests cost as much as the exact tests they save), off
    bool film_fused = true;    // the path integrator's k_raygen writes the radiance records in the film pass's layout with their splat descriptors (no memset, no pack pass; option "film_fused")
    bool trace3_spec = true;   // k_trace3 (closest-hit): lanes park the leaf they reach and go on descending (th_trace2.h, TH_TRACE3_SPEC); 0 = wait for the leaf phase
    bool hybrid = true;        // scenes committed with both trees (bvh_builder 4 / -1): closest-hit rays walk the ACCELERATOR with the order-independence certificate of
                               // th_trace3c.h and only the flagged ones the canonical tree (option "hybrid"; 0 = every ray walks the canonical tree: same answers, slower)
    bool trace7_cheap = true;  // k_trace7: conservative fma slab test on interior boxes, the reference's exact test once per leaf (th_trace7.h); 0 = exact test on every box
    int streaming = 0;             // PathIntegrator on scenes with a real hierarchy: suspend / resume stragglers.  1 = always, 0 = never (classic
                                   // per-depth launches), -1 = automatic: when the frame has at most 96 camera samples per primitive, which is where the
                                   // traversal tails dominate (measured, 1 M triangles: 16 spp 1170 -> 716 ms, 64 spp 1700 -> 1443, 128 spp 2288 vs
                                   // 2412, 256 spp 3742 vs 3823; 10 M triangles, depth 16: 32 spp 6075 -> 2465 ms, 128 spp 8364 -> 4913)
    uint32_t stream_budget_shift = 12;  // budget = max(stream_budget_min, fresh rays of the round >> shift)
    uint32_t stream_list_cap = 0;       // suspended-ray list capacity (0 = max(65536, paths / 128)); tests shrink it
    uint32_t stream_budget_min = 2048;  // interior fetches before a ray may be suspended (tests lower it to force suspensions)
    uint64_t sppm_batch = 0;  // SPPM iterations per wavefront batch (0 = from free HBM, at most 128)
    int denoise_lds = 3;    // bit i: iteration i (step 2^i, i < 2) of trhip_denoise runs the LDS-staged kernel (option "denoise_lds")
    int temporal_patch = 1; // trhip_temporal's lane-to-pixel mapping: 0 film order, 1 patches of 16 x 4 per wave, measured 11 % faster (option "temporal_patch", profiles/r11/temporal.txt)
    int denoise_var_lds = 3;  // bit i: iteration i (step 2^i, i < 2) of trhip_denoise_var runs the LDS-staged kernel (option "denoise_var_lds", profiles/r13/variance.txt)
};

// How a value becomes its field.  Flag: value != 0.  Tri: value < 0 -> -1, else value != 0.  Clamp: into [lo, hi].  Mask3: value & 3.  Cast: as it is.  Range: values
// outside [lo, hi] are refused with the row's sentence.  RangeBut5: Range, and 5 is refused too.  What comes out is cast to the field's type.
enum class OptionRule { Flag, Tri, Clamp, Mask3, Cast, Range, RangeBut5 };
struct OptionField {  // a member of Options, written with the cast to its type and read back (the host test reads)
    void (*store)(Options&, int64_t);
    int64_t (*load)(const Options&);
};
template <auto M>
constexpr OptionField at() {
    return {[](Options& o, int64_t v) { o.*M = static_cast<std::decay_t<decltype(o.*M)>>(v); }, [](const Options& o) { return (int64_t)(o.*M); }};
}
// Kernel families that lost their measurements (traversals 4 / 6 / 7, the leaf queue, the sorted one-leaf walk, the linear BVH builder) are compiled only with
// -DTRHIP_EXPERIMENTS (__graft_entry__.build_library(extra_flags=["-DTRHIP_EXPERIMENTS"], out_name="libtracehip_experiments.so")); the default library refuses their options.
// A row names them in `needs`: bit v is set when the value that WOULD be stored, v, exists only in that build; `needs_what` begins the refusal (a %d is the value).
struct OptionRow {
    const char* name;
    OptionRule rule;
    OptionField field;
    int64_t lo = 0, hi = 0;
    const char* refusal = nullptr;  // Range / RangeBut5: the sentence for a value outside (a %d is hi)
    uint32_t needs = 0;
    const char* needs_what = nullptr;
};
constexpr int64_t kOptionNoMax = INT64_MAX;
inline const char* const kNeedsExperiments = "needs the EXPERIMENTS build of the library (-DTRHIP_EXPERIMENTS): not in the default binary";

inline const OptionRow kOptionRows[] = {
    {"count_visits", OptionRule::Flag, at<&Options::count_visits>()},
    {"timing", OptionRule::Flag, at<&Options::timing>()},
    {"debug_trace_budget", OptionRule::Cast, at<&Options::debug_trace_budget>()},
    {"streaming", OptionRule::Tri, at<&Options::streaming>()},
    {"stream_budget_shift", OptionRule::Clamp, at<&Options::stream_budget_shift>(), 0, 31},
    {"stream_list_cap", OptionRule::Clamp, at<&Options::stream_list_cap>(), 0, kOptionNoMax},
    {"stream_budget_min", OptionRule::Clamp, at<&Options::stream_budget_min>(), 1, kOptionNoMax},
    {"sppm_batch", OptionRule::Clamp, at<&Options::sppm_batch>(), 0, kOptionNoMax},
    {"bvh_builder", OptionRule::Clamp, at<&Options::bvh_builder>(), -1, 4, nullptr, 1u << 1, "bvh_builder = 1 (the linear BVH)"},
    {"hybrid", OptionRule::Flag, at<&Options::hybrid>()},
    {"band_tile_rows", OptionRule::Clamp, at<&Options::band_tile_rows>(), 0, kOptionNoMax},
    {"compose_spheres", OptionRule::Tri, at<&Options::compose_spheres>()},
    {"occluder_pretest", OptionRule::Flag, at<&Options::occluder_pretest>()},
    {"stream2_priority", OptionRule::Cast, at<&Options::stream2_priority>()},
    {"leaf_sorted", OptionRule::Flag, at<&Options::leaf_sorted>(), 0, 0, nullptr, 1u << 1, "leaf_sorted"},
    {"film_fused", OptionRule::Flag, at<&Options::film_fused>()},
    {"trace3_spec", OptionRule::Flag, at<&Options::trace3_spec>()},
    {"trace7_cheap", OptionRule::Flag, at<&Options::trace7_cheap>()},
    {"leaf_kernel", OptionRule::Flag, at<&Options::leaf_kernel>()},
    {"slab_margin_log2", OptionRule::Clamp, at<&Options::slab_margin_log2>(), 0, 20},
    {"tiny_scene_prims", OptionRule::Clamp, at<&Options::tiny_scene_prims>(), 0, 255},
    {"film_relayout", OptionRule::Flag, at<&Options::film_relayout>()},
    {"any_on_accelerator", OptionRule::Tri, at<&Options::any_on_accelerator>()},
    {"leaf_queue", OptionRule::Flag, at<&Options::leaf_queue>(), 0, 0, nullptr, 1u << 1, "leaf_queue"},
    {"wide4", OptionRule::Flag, at<&Options::wide4>()},
    {"node_layout", OptionRule::Range, at<&Options::node_layout>(), 0, 1, "node_layout: 0 (depth-first) or 1 (sibling pairs per 128-byte line)"},
    {"denoise_lds", OptionRule::Mask3, at<&Options::denoise_lds>()},
    {"temporal_patch", OptionRule::Flag, at<&Options::temporal_patch>()},
    {"denoise_var_lds", OptionRule::Mask3, at<&Options::denoise_var_lds>()},
    {"pipelines", OptionRule::Range, at<&Options::pipelines>(), 1, kMaxPipes, "pipelines must be in 1..%d"},
    {"overlap", OptionRule::Flag, at<&Options::overlap>()},
    {"traversal", OptionRule::RangeBut5, at<&Options::traversal>(), 1, 7, "traversal must be 1, 2, 3, 4, 6 or 7", 1u << 4 | 1u << 6 | 1u << 7, "traversal %d"},
    {"batch_paths", OptionRule::Range, at<&Options::batch_paths>(), 0, kOptionNoMax, "batch_paths must be >= 0 (0 = auto)"},
};

inline const OptionRow* find_option(const char* name) {
    for (const OptionRow& r : kOptionRows)
        if (!std::strcmp(name, r.name)) return &r;
    return nullptr;
}
inline int64_t option_stored(const OptionRow& r, int64_t value) {  // what the row's rule makes of a value (before the cast)
    switch (r.rule) {
    case OptionRule::Flag: return value != 0;
    case OptionRule::Tri: return value < 0 ? -1 : (value != 0 ? 1 : 0);
    case OptionRule::Clamp: return std::max<int64_t>(r.lo, std::min<int64_t>(r.hi, value));
    case OptionRule::Mask3: return value & 3;
    default: return value;
    }
}
// does this build carry `name = value`?  (A name the table does not know is nobody's to refuse: yes.)
inline bool option_in_build(bool experiments_build, const char* name, int64_t value) {
    const OptionRow* r = find_option(name);
    if (experiments_build || !r) return true;
    const int64_t v = option_stored(*r, value);
    return !(v >= 0 && v < 32 && (r->needs >> v & 1u));
}
// The only interpreter of the table: 0 and the field written, or a TRHIP_ERR_ code, its sentence in msg and the field as it was.  A value out of a row's range is
// refused before the build is asked.
inline int apply_option(Options& opt, bool experiments_build, const char* name, int64_t value, char* msg, size_t n) {
    const OptionRow* r = find_option(name);
    if (!r) {
        std::snprintf(msg, n, "unknown option %s", name);
        return TRHIP_ERR_INVALID;
    }
    const bool ranged = r->rule == OptionRule::Range || r->rule == OptionRule::RangeBut5;
    if (ranged && (value < r->lo || value > r->hi || (r->rule == OptionRule::RangeBut5 && value == 5))) {
        std::snprintf(msg, n, r->refusal, (int)r->hi);
        return TRHIP_ERR_INVALID;
    }
    if (!option_in_build(experiments_build, name, value)) {
        const int at = std::snprintf(msg, n, r->needs_what, (int)value);
        std::snprintf(msg + at, n - at, " %s", kNeedsExperiments);
        return TRHIP_ERR_UNSUPPORTED;
    }
    r->field.store(opt, option_stored(*r, value));
    return 0;
}
