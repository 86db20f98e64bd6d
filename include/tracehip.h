/* tracehip.h — C ABI of libtracehip.so, the MI355X (gfx950) wavefront ray/path-tracing engine behind Trace.jl's
 * Integrator / Sampler / Film surface.
 *
 * The reference (pxl-th/Trace.jl @ 2024_10_08) has no FFI layer: its "operator API" is Julia dispatch on a handful of
 * types.  Each entry point below names the reference interface (file:line under /root/reference/src)
 * it replaces.  A Julia shim (trace.jl_amd/julia/TraceHIP.jl) `ccall`s these after walking
 * Scene -> BVHAccel -> GeometricPrimitive; the tested host in this repo is the Python mirror in trace.jl_amd/.
 *
 * Conventions: every function returns 0 on success and a negative trhip_status on failure; the message is available
 * from trhip_last_error().  Nothing throws across the boundary.  Host pointers are caller-owned and only borrowed for
 * the duration of the call.  Calls are blocking (internal HIP streams are synchronised before returning).  One
 * trhip_ctx owns one GPU; use one process per GPU.  Several processes form one job through trhip_comm_init (RCCL over xGMI):
 * trhip_film_reduce sums the per-rank film accumulators, trhip_render_sppm shards its photons (multi-GPU section below).
 * Matrices are 16 floats, row-major: m[4*row + col] (Julia's Mat4f is column-major: pass transpose / permutedims).
 * All arithmetic is IEEE Float32 without FMA contraction; transcendental functions and the sampler are the ones
 * specified in trace_detmath.h / trace_sampler.h, so results are reproducible bit-for-bit on any conforming host.
 */
#ifndef TRACEHIP_H
#define TRACEHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trhip_ctx trhip_ctx;
typedef struct trhip_scene trhip_scene;

typedef enum {
    TRHIP_OK = 0,
    TRHIP_ERR_INVALID = -1,    /* bad argument / call order */
    TRHIP_ERR_HIP = -2,        /* HIP runtime error (no device, out of memory, launch failure) */
    TRHIP_ERR_UNSUPPORTED = -3 /* feature of the reference that this build does not accelerate */
} trhip_status;

/* ---- context ------------------------------------------------------------------------------------------------------- */
/* Fails (TRHIP_ERR_HIP) when no gfx950 device is visible: there is no CPU fallback. */
int trhip_init(trhip_ctx** ctx, int device_id);
void trhip_shutdown(trhip_ctx* ctx);
/* ctx may be NULL to read the message of a failed trhip_init. */
const char* trhip_last_error(const trhip_ctx* ctx);
/* ABI version of this header: major*1000 + minor. */
int trhip_version(void);  /* 3001 */

/* ---- scene flattening (replaces the Scene / BVHAccel / GeometricPrimitive object graph) --------------------------- */
/* Scene(lights, aggregate)  Trace.jl:176-187 */
int trhip_scene_new(trhip_ctx* ctx, trhip_scene** out);
void trhip_scene_free(trhip_scene* scene);

/* Materials with ConstantTexture arguments (textures/basic.jl:4-10), materials/material.jl:
 *   TRHIP_MATTE   (:1-31)    params = Kd.rgb, sigma                                           (4)
 *   TRHIP_MIRROR  (:34-46)   params = Kr.rgb                                                  (3)
 *   TRHIP_GLASS   (:49-116)  params = Kr.rgb, Kt.rgb, u_roughness, v_roughness, index, remap  (10)
 *   TRHIP_PLASTIC (:119-151) params = Kd.rgb, Ks.rgb, roughness, remap                        (8) */
enum { TRHIP_MATTE = 0, TRHIP_MIRROR = 1, TRHIP_GLASS = 2, TRHIP_PLASTIC = 3 };
int trhip_scene_add_material(trhip_scene* scene, int kind, const float* params, int n_params, uint32_t* id_out);

/* create_triangle_mesh + one GeometricPrimitive per triangle  (shapes/triangle_mesh.jl:45-58, primitive.jl:5-9).
 * world_xyz: vertices already moved to world space by the host exactly as TriangleMesh does (triangle_mesh.jl:23);
 * normals are passed untransformed (triangle_mesh.jl:23-28) or NULL; indices are 1-based as in the reference;
 * flip_orientation = reverse_orientation XOR transform_swaps_handedness of the ShapeCore (shapes/Shape.jl:7-14);
 * material_id_per_tri may be NULL only for geometry-only scenes (kernel-level trace entry points).
 * first_prim_out receives the index of the first created primitive in caller order. */
int trhip_scene_add_triangles(trhip_scene* scene, const float* world_xyz, uint32_t n_verts, const uint32_t* indices_1based, uint32_t n_tris,
                              const float* normals_or_null, const uint32_t* material_id_per_tri, int flip_orientation, uint32_t* first_prim_out);

/* The same with the mesh's two optional per-vertex arrays (shapes/triangle_mesh.jl:1-30, create_triangle_mesh's last two arguments):
 * tangents: n_verts x 3, untransformed like the normals, read through the indices (:76-78) — the shading tangent of a hit is their barycentric
 *   mix (:172-176) instead of ∂p∂u; a mesh with tangents and no normals still gets shading geometry (:165);
 * uv: the reference reads `mesh.uv[t.i + j]` (:82) — indexed by the triangle's CORNER position 3k + j in the index list, not through the indices —
 *   so the array holds 3 x n_tris points (2 floats each), corner-major; ∂p∂u / ∂p∂v (:125-141) and interaction.uv follow from it.
 * Either pointer may be NULL (both NULL = trhip_scene_add_triangles). */
int trhip_scene_add_triangles_ex(trhip_scene* scene, const float* world_xyz, uint32_t n_verts, const uint32_t* indices_1based, uint32_t n_tris,
                                 const float* normals_or_null, const float* tangents_or_null, const float* uv_corners_or_null,
                                 const uint32_t* material_id_per_tri, int flip_orientation, uint32_t* first_prim_out);

/* Sphere(core, radius, z_min, z_max, ϕ_max°) + GeometricPrimitive  (shapes/sphere.jl:1-30).  Both matrices of
 * core.object_to_world (m and inv_m, transformations.jl:1-4) are passed because the reference keeps them separately
 * (and multiplies inverses in a non-standard order, transformations.jl:20-22). */
int trhip_scene_add_sphere(trhip_scene* scene, const float obj2world_m[16], const float obj2world_inv_m[16], int reverse_orientation, float radius,
                           float z_min, float z_max, float phi_max_deg, uint32_t material_id, uint32_t* prim_out);

/* Same, for hosts that hold an already constructed Trace.Sphere (the Julia shim): the fields exactly as the reference's
 * constructor derived them (sphere.jl:13-26: clamped z_min/z_max, θ_min, θ_max, ϕ_max in radians), so that no
 * elementary function is re-evaluated on this side of the boundary. */
int trhip_scene_add_sphere_fields(trhip_scene* scene, const float obj2world_m[16], const float obj2world_inv_m[16], int reverse_orientation, float radius,
                                  float z_min, float z_max, float theta_min, float theta_max, float phi_max_rad, uint32_t material_id, uint32_t* prim_out);

/* PointLight(light_to_world, I)  lights/point.jl:19-24 ;  SpotLight(light_to_world, I, total°, falloff_start°)  lights/spot.jl:10-19 */
int trhip_scene_add_point_light(trhip_scene* scene, const float light2world_m[16], const float light2world_inv_m[16], const float I[3]);
int trhip_scene_add_spot_light(trhip_scene* scene, const float light2world_m[16], const float light2world_inv_m[16], const float I[3],
                               float total_width_deg, float falloff_start_deg);

/* SpotLight from its constructed fields (cos_total_width, cos_falloff_start; lights/spot.jl:1-8). */
int trhip_scene_add_spot_light_fields(trhip_scene* scene, const float light2world_m[16], const float light2world_inv_m[16], const float I[3],
                                      float cos_total_width, float cos_falloff_start);

/* DirectionalLight(light_to_world, I, direction)  lights/directional.jl:6-33, from the fields the light holds at render time:
 * direction_world = normalize(light_to_world(direction)) (:29, a vector: translation ignored) and world_radius (0 after the
 * constructor, the scene's bounding sphere after preprocess!(light, scene) :35-37; Scene never calls it, Trace.jl:184).  The
 * library does not preprocess: what the caller's light holds is what renders.  sample_li (:39-47): Li = I, wi = direction, pdf 1,
 * shadow ray spawn_ray(p, p .+ direction .* (2 * world_radius)) — with world_radius 0 a zero-direction ray.  SPPM refuses a call
 * whose photon pass could pick the light (the reference has no sample_le for it, sppm.jl:361): see trhip_render_sppm. */
int trhip_scene_add_directional_light(trhip_scene* scene, const float I[3], const float direction_world[3], float world_radius);

/* BVHAccel(primitives, max_node_primitives)  accel/bvh.jl:55-79.  Builds a binned-SAH BVH2 on the host (results of
 * traversal do not depend on the topology except where two primitives are accepted at (nearly) the same t), flattens it
 * in the reference's depth-first layout (first child = i+1, bvh.jl:187-206) and uploads everything to HBM.  Option "bvh_builder" = 2
 * builds the reference's OWN tree instead (its 12-bucket construction, quirks included): same tie-breaks as Trace.jl; a host that
 * already holds Trace.jl's BVHAccel hands its nodes over with trhip_scene_set_bvh (what TraceHIP.jl does). */
int trhip_scene_commit(trhip_scene* scene, int max_node_primitives);

/* A relit view of a committed scene: Scene(new_lights, the same BVHAccel) without building its geometry again.  *out shares `base`'s committed geometry (trees, primitive
 * and shading records, materials, the accelerator and its certificate data), belongs to base's context, starts with NO lights and is not committed.  Add lights with
 * trhip_scene_add_*_light, then trhip_scene_commit(*out, max_node_primitives): on a view it runs only the light stage (uploads the lights and orders the any-hit tests by
 * them) and max_node_primitives must be what the geometry was committed with.  Renders on the view return, bit for bit, what a fresh commit of the same primitives with
 * those lights returns.  A relit view can be relit in turn (same geometry).  The geometry is reference-counted: freeing base leaves its views working.  Committing base
 * again (after adding primitives or materials, say) gives base new geometry; earlier views keep theirs.  Context options read at commit time do not apply to a view: it
 * has its base's trees, trhip_scene_bvh_mode and trhip_scene_bvh_note.  On a view, adding materials or primitives and trhip_scene_set_bvh are refused
 * (TRHIP_ERR_INVALID), and so is trhip_scene_set_bvh on a scene whose geometry a live view still shares.  TRHIP_ERR_INVALID when base is not committed. */
int trhip_scene_relight(const trhip_scene* base, trhip_scene** out);
/* An identifier of the committed geometry a handle holds: two handles return the same id exactly when they share it (0: never committed). */
int trhip_scene_geometry_id(const trhip_scene* scene, uint64_t* id);

/* BVHAccel construction alone, on the host (no GPU needed): builder 0 = the library's binned SAH, 2 = the REFERENCE's construction node for node
 * (accel/bvh.jl:87-206 + partition! Trace.jl:128-137, quirks kept — SURVEY.md A.6; what trhip_scene_commit builds under option "bvh_builder" = 2).
 * prim_bounds: n_prims * 6 (world_bound of each primitive: min xyz, max xyz).  Outputs in the layout of trhip_scene_get_bvh; *n_nodes_inout = capacity
 * of the node arrays on entry, the tree's node count on return (all output pointers NULL: size query).  The reference's builder may emit leaves of 0
 * primitives with bounds (+Inf, -Inf): up to ~3 n nodes.  TRHIP_ERR_UNSUPPORTED where the reference's recursion would not end. */
int trhip_build_bvh_host(int builder, const float* prim_bounds, uint32_t n_prims, int max_node_primitives, float* node_bounds, uint32_t* node_a, uint32_t* node_flags,
                         uint32_t* n_nodes_inout, uint32_t* prim_order, uint32_t* max_depth_out);

/* Inspection of the committed BVH (tests feed the same topology to the CPU oracle so that parity is bit-exact).
 * node_bounds: n_nodes*6 (min xyz, max xyz).  Leaf: (flags & 3) == 3, a = first ordered-primitive slot, n = flags >> 2.
 * Interior: a = index of the second child, flags & 3 = split axis (0..2), first child = i + 1.
 * prim_order[slot] = caller primitive index.  Any output pointer may be NULL. */
int trhip_scene_bvh_size(const trhip_scene* scene, uint32_t* n_nodes, uint32_t* n_prims);
int trhip_scene_get_bvh(const trhip_scene* scene, float* node_bounds, uint32_t* node_a, uint32_t* node_flags, uint32_t* prim_order);
/* Replace the BVH by a caller-supplied one in the same layout (e.g. the reference's own builder run elsewhere). */
int trhip_scene_set_bvh(trhip_scene* scene, const float* node_bounds, const uint32_t* node_a, const uint32_t* node_flags, uint32_t n_nodes,
                        const uint32_t* prim_order, uint32_t n_prims);

/* Hybrid mode (option "bvh_builder" = 4, and the default): the scene holds TWO trees over the same primitives.  The CANONICAL one — the reference's own construction
 * (accel/bvh.jl:55-206, or the tree a host handed to trhip_scene_set_bvh) — defines the answers: slots, trhip_scene_get_bvh, shading records are its.  The library's
 * binned-SAH tree rides along as the ACCELERATOR: closest-hit rays walk it and carry a certificate that every valid tree over the same leaves returns the same hit;
 * rays without the certificate (a sphere entered from inside, sphere.jl:137-138; two acceptable primitives within 512 ulps of the ray's reach; a grazed leaf box;
 * a zero direction component) are re-walked on the canonical tree in the reference's order (trhip_stats.fallback_rays).  Results equal a walk of the canonical tree
 * alone bit for bit (option "hybrid" = 0 runs exactly that walk, for A/B).
 * trhip_scene_bvh_mode: *mode = 0 the library's tree alone (bvh_builder 0 / 1 / 3), 1 the canonical tree alone (bvh_builder 2; or a scene whose accelerator could not be
 *   certified: leaf boxes that differ between the trees), 2 both, 3 the library's tree as the canonical tree AND, four children wide, as its own accelerator (a default
 *   commit on a scene where the reference's construction fails: trhip_scene_bvh_note says why); *accel_nodes / *accel_depth describe the accelerator (0 without one).
 * trhip_scene_get_accelerator: the accelerator in the layout of trhip_scene_get_bvh (prim_order[accelerator slot] = caller primitive index); size it with
 *   trhip_scene_bvh_mode.  Any output pointer may be NULL. */
int trhip_scene_bvh_mode(const trhip_scene* scene, int* mode, uint32_t* accel_nodes, uint32_t* accel_depth);
/* The name of the kernel a closest-hit launch on this scene runs under the context's current options ("k_trace3c4": the certified walk on the accelerator four children wide,
 * "k_trace3c": the same on the binary accelerator — wide4 = 0, or an accelerator whose four-wide form does not fit the stack —, "k_trace_leaf_c": a one-leaf accelerator, "k_trace3",
 * "k_trace_leaf", …): for profile filters and rooflines, which must name the kernel that ran. */
int trhip_closest_kernel_name(const trhip_ctx* ctx, const trhip_scene* scene, char* buf, size_t n);
/* Why a scene committed with default options holds ONE tree (mode 0 or 1) instead of two: a NUL-terminated sentence copied into buf (at most n bytes; "" for mode 2 and for
 * explicit builders).  E.g. "the reference's construction: BVH depth 71 exceeds the 64-entry traversal stack (bvh.jl:222 throws a BoundsError there)" -> the library's tree alone. */
int trhip_scene_bvh_note(const trhip_scene* scene, char* buf, size_t n);
/* Why a scene that holds both trees is walked WITHOUT its accelerator under the context's current options ("" when it is used, or the scene holds one tree): such frames
 * are exact but walk the reference's tree alone, at about twice the closest-hit time.  The first such frame of a context also says so on stderr.  Also non-empty when the
 * accelerator IS used but the last frame that reported statistics handed more than a fifth of its closest-hit rays back to the reference-order walk (trhip_stats.fallback_rays /
 * closest_rays: scenes of near-ties — tiny coplanar triangles, rays in a primitive's plane): exact, at little gain; that frame says so once on stderr as well. */
int trhip_accelerator_note(const trhip_ctx* ctx, const trhip_scene* scene, char* buf, size_t n);
int trhip_scene_get_accelerator(const trhip_scene* scene, float* node_bounds, uint32_t* node_a, uint32_t* node_flags, uint32_t* prim_order);

/* ---- sensor: PerspectiveCamera + Film + filter (camera/perspective.jl:58-80, film.jl:34-61, filter.jl) ------------- */
typedef struct {
    float raster_to_camera[16]; /* camera.core.raster_to_camera.m — composed by the host constructors, bugs included (A.3, A.4) */
    float camera_to_world[16];  /* camera.core.core.camera_to_world.m */
    float lens_radius, focal_distance, shutter_open, shutter_close;
    float crop_min[2], crop_max[2]; /* Film.crop_bounds: 1-based inclusive pixel bounds (film.jl:41-44) */
    float filter_radius[2];         /* Film.filter.radius */
    float filter_table[256];        /* Film.filter_table, (y, x) order: table[16*y + x] (film.jl:38-40, 55-59) */
    float scale;                    /* Film.scale */
} trhip_sensor;

typedef struct {
    uint64_t camera_samples; /* camera samples completed */
    uint64_t closest_rays;   /* closest-hit rays traced, all bounces */
    uint64_t shadow_rays;    /* any-hit (shadow) rays traced, all bounces */
    uint64_t nodes_visited;  /* filled only when instrumentation is on (trhip_set_option "count_visits") */
    uint64_t prims_tested;
    uint64_t nodes_visited_shadow; /* any-hit rays: box and primitive RECORDS fetched — a record one scalar fetch brings to all 64 rays of */
    uint64_t prims_tested_shadow;  /* a wave (the any-hit pre-pass kernels of th_trace2.h) counts once                                   */
    double ms_total;         /* wall time of the render call's device work (HIP events) */
    double ms_raygen, ms_trace_closest, ms_shade, ms_trace_any, ms_film;
    uint32_t launches_raygen, launches_trace_closest, launches_shade, launches_trace_any, launches_film;
    uint32_t n_batches, max_depth_reached;
    uint32_t traversal;      /* traversal kernel that ran: 1 literal, 2, 3 binary children-in-parent walk, 4 8-wide nodes, 5 one-leaf scene, 9 hybrid: the certified
                                walk on the accelerator tree + the reference-order walk of the rays it hands back (trhip_scene_bvh_mode) */
    uint32_t node_bytes;     /* bytes fetched per unit of nodes_visited: 32 (a node box of the binary kernels: 64-byte node = 2 boxes),
                                96 (one 8-wide node: six 16-byte loads from one 128-byte line), 0 (one-leaf scene: scalar loads) */
    /* ---- since ABI 3000 ---- */
    uint64_t replicated_rays; /* of closest_rays + shadow_rays: rays that EVERY rank of a multi-GPU job traces identically (the camera pass of
                                 trhip_render_sppm, which only shards its photons); a job's ray total counts them once */
    uint64_t fallback_rays;   /* closest-hit rays the order-free walk (traversal 7) flagged — a second candidate within the tie margin, a box it
                                 could not decide, an origin inside a sphere — and handed to the reference-order walk (k_trace3) */
    double ms_sub[4];         /* parts of ms_shade.  trhip_render_sppm: [0] photon gather (k_sppm_gather + k_sppm_gather_hot), [1] camera / photon
                                 shading, [2] grid bounds + hit binning + scans, [3] pixel update + fold.  Path / Whitted: zeros */
    uint32_t launches_sub[4];
    uint64_t count_sub[4];    /* trhip_render_sppm with "count_visits": [0] (pixel, photon) candidates distance-tested by the gather, [1] pairs accepted
                                 (BSDF evaluated), [2] photon hits binned, [3] visible points.  trhip_render_path with traversal 7 and "count_visits": why rays went to
                                 the reference-order walk — [0] zero / non-finite direction, [1] a sphere (origin inside, limb, clipped), [2] a candidate within the gap of
                                 the ray's own t_max, [3] a second candidate within the gap of the nearest.  Hybrid mode (traversal 9) with "count_visits": why rays went to the
                                 canonical tree — [0] a zero / non-finite direction component or a near-axis-parallel direction, [1] a sphere (clipped; inside two at once),
                                 [2] a candidate within 2 dt of the incumbent or before its own leaf box's entry; and, NOT a fallback, [3] rays that start inside a sphere and were
                                 certified on the accelerator (sphere.jl:137-138 handled through the order word).  Otherwise zeros */
    /* ---- since ABI 3001: hybrid mode (traversal 9).  Of ms_trace_closest / nodes_visited / prims_tested, the part of the FALLBACK walks (k_trace3 over the rays the
       certified walk handed back, on the canonical tree); the certified walk on the accelerator tree (k_trace3c) is the difference ---- */
    double ms_fallback;
    uint32_t launches_fallback, reserved0;
    uint64_t nodes_visited_fallback, prims_tested_fallback;
} trhip_stats;

/* How trhip_render_path splits a frame whose per-sample buffers do not fit into `budget_bytes` (host arithmetic, no GPU): bands of whole rows of 16 x 16 sample tiles
 * (integrators/sampler.jl:15-24: tiles in k order — bands are ranges of k, so the film is the sequential loop's bit for bit).  bytes_per_sample: 17 (radiance record + poison byte: the
 * default film pass), 25 or 33 with the other film passes.  Writes up to `cap` bands: first sample row (film coordinates) and number of sample rows; *n_bands = how many there are. */
int trhip_plan_bands(const trhip_sensor* sensor, uint32_t spp, uint64_t budget_bytes, uint32_t bytes_per_sample, uint32_t cap, uint32_t* n_bands, int32_t* first_row, int32_t* n_rows);

/* ---- integrators (replace `integrator(scene)`, integrators/sampler.jl:12-56) ---------------------------------------
 * out_xyzw: (crop height) * (crop width) * 4 floats in film.pixels (y, x) order = Pixel.xyz sums + filter_weight_sum
 * (film.jl:7-11), i.e. exactly the state `save(film)` (film.jl:204-222) starts from.  NaN radiance samples are zeroed
 * (integrators/sampler.jl:46).  The sampler is the seeded counter-based sampler of trace_sampler.h with
 * `samples_per_pixel = spp`; `sample_offset` shifts the global sample indices (rank r of an N-GPU job renders indices
 * [r*spp, (r+1)*spp) and the host sum-reduces the films).
 * The *_device variants write to a DEVICE pointer (e.g. a torch tensor's data_ptr) instead of host memory. */
int trhip_render_whitted(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed,
                         uint32_t sample_offset, float* out_xyzw, trhip_stats* stats);
/* PathIntegrator: not in the reference; defined in DESIGN.md from integrators/sppm.jl:208-266, 503-554. */
int trhip_render_path(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed,
                      uint32_t sample_offset, float* out_xyzw, trhip_stats* stats);
int trhip_render_path_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed,
                             uint32_t sample_offset, void* d_out_xyzw, trhip_stats* stats);
int trhip_render_whitted_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed,
                                uint32_t sample_offset, void* d_out_xyzw, trhip_stats* stats);
/* Per-sample radiance of the last render call (after the NaN rule), n_sample_pixels * spp * 3 floats indexed
 * [(s * n_sample_pixels + (y - sb.min.y) * sb_width + (x - sb.min.x)) * 3 + c]; sample bounds sb = get_sample_bounds(film)
 * (film.jl:68-73).  Parity tests compare this with the oracle bit-for-bit. */
int trhip_last_sample_radiance(trhip_ctx* ctx, float* out_rgb, uint64_t n_floats);

/* ---- adaptive sampling (added without a version change: nothing existing moved; docs/design/24-adaptive.md is the specification) -------
 * trhip_render_path_map: trhip_render_path with a per-pixel sample count instead of one spp.
 *   counts     one uint32 per SAMPLE pixel — the film's sample bounds, filter border included — indexed like trhip_last_sample_radiance:
 *              (y - sb.min.y) * sb_width + (x - sb.min.x); every entry in 0 .. max_spp.
 * Sample pixel p draws the sample indices sample_offset + s for s < counts[p] and no others.  ts_stream_key (trace_sampler.h) does not depend on
 * the sample count, so each drawn sample's radiance is trhip_render_path's for that (pixel, index) bit for bit.  The film is the reference loop
 * (integrators/sampler.jl:24-52, film.jl:134-193) with samples_per_pixel replaced by counts[p]: tiles in k order, sample pixels in Bounds2
 * order, samples in index order, one partial sum per tile, the NaN rule; a sample that is not drawn is SKIPPED, not added with weight 0.
 * counts == spp everywhere is trhip_render_path(spp) bit for bit, and films stay additive over sample_offset.
 * Work: stats.camera_samples = sum of counts; no ray is generated for a sample that is not drawn and the film pass reads no record of one.
 * The frame's camera samples are a job list (an exclusive sum over counts, then one word per drawn sample, 4 bytes each); wavefront batches are
 * ranges of that list.  The sum of counts plans the batches on the host: the host variant adds the counts up on the host, the _device variant
 * reads 8 bytes back after a reduction over the map on the device.
 * Film passes: a filter radius in (0, 1] on both axes takes the pixel-group-major records with packed splat descriptors and the 2 x 4 gather;
 * any other radius takes sample-major records, film positions for the drawn samples and the 1 x 4 block gather.  The options that select other
 * record paths into the film pass ("film_fused", "film_relayout"), "streaming" and "pipelines" are
 * IGNORED by map frames; "batch_paths" (rounded down to whole waves of 64) and "overlap" hold.
 * trhip_last_sample_radiance after a map frame: the dense max_spp * n_sample_pixels * 3 array, +0.0 in every entry with s >= counts[p].
 * TRHIP_ERR_INVALID, in this order: a null pointer (stats excepted); max_spp == 0; an empty film; a count above max_spp (looked for on the host
 * by the host variant, on the device beside the sum by the _device variant); a sum of counts of 0; then trhip_render_path's refusals in its
 * order (an uncommitted scene, max_depth).  TRHIP_ERR_UNSUPPORTED: 2^31 sample pixels or 2^32 camera samples at max_spp (after the empty
 * film); a scene with a material-less primitive, where trhip_render_path refuses it; a frame whose per-sample buffers — dense at max_spp, 17 or
 * 25 bytes per slot, and 4 bytes per drawn sample — do not fit in half of free HBM: there are no bands here, as in trhip_render_aov.
 * The _device variant takes DEVICE pointers for counts and the film. */
int trhip_render_path_map(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, const uint32_t* counts, uint32_t max_spp, int max_depth, uint64_t seed,
                          uint32_t sample_offset, float* out_xyzw, trhip_stats* stats);
int trhip_render_path_map_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, const void* d_counts, uint32_t max_spp, int max_depth, uint64_t seed,
                                 uint32_t sample_offset, void* d_out_xyzw, trhip_stats* stats);

/* trhip_film_sum: out = a + b on all FOUR lanes, one Float32 addition each, for two films of height * width * 4 floats: the film of sample indices [o, o + n0)
 * plus a map frame's film at sample_offset o + n0 is the film of their union up to the order of the two partial sums, weight lane included.  (trhip_film_add keeps
 * a's weight lane and is not the call for this.)  out may be a or b.  TRHIP_ERR_INVALID: a null pointer; a zero dimension.  The _device variant takes DEVICE pointers
 * and allocates nothing. */
int trhip_film_sum(trhip_ctx* ctx, const float* a, const float* b, uint32_t width, uint32_t height, float* out);
int trhip_film_sum_device(trhip_ctx* ctx, const void* d_a, const void* d_b, uint32_t width, uint32_t height, void* d_out);

/* trhip_last_sample_stats: mean and variance of the luminance of every sample pixel over the n = spp radiance records of the context's last
 * one-band trhip_render_path frame (either record layout), or over the records the last trhip_film_accumulate was given.  out_mv: n_sample_pixels * 2 floats, (m, v) per sample pixel in
 * trhip_last_sample_radiance's pixel order.  Per sample, in index order: the NaN rule (a record with a NaN lane counts as black),
 * Y = 0.212671 r + 0.715160 g + 0.072169 b evaluated left to right, S1 += Y, S2 += Y * Y, both from +0; then m = S1 / n,
 * x = S2 / n - m * m, v = x < 0 ? +0 : x (a NaN x stays NaN).  All Float32, no contraction.
 * TRHIP_ERR_INVALID: a null pointer; a last frame that is neither (none yet, a banded, Whitted, AO or map frame). */
int trhip_last_sample_stats(trhip_ctx* ctx, float* out_mv);
int trhip_last_sample_stats_device(trhip_ctx* ctx, void* d_out_mv);

/* trhip_sample_map: the extra samples per sample pixel that bring the relative standard error of a pilot frame's own estimate under tau.
 *   mv           sb_height * sb_width * 2 floats: what trhip_last_sample_stats wrote for a pilot frame of `pilot` samples per pixel
 *   out_counts   sb_height * sb_width uint32;  out_total: one uint64, the sum of out_counts (an integer sum: no order in it)
 * e[q] = v / ((|m| + eps) * (|m| + eps)), +Inf when that is NaN or not finite;  E[p] = the largest e over the 3 x 3 sample pixels around p
 * that lie inside the sample bounds;  x = E / (tau * tau);  counts[p] = max_extra when !(x < float(pilot + max_extra)), otherwise
 * max(0, int(ceilf(x)) - pilot).  A relative-error target measured on the pilot's own samples is biased, like every such scheme
 * (docs/design/24-adaptive.md); adding the map frame to the pilot frame keeps every pixel's pilot samples.
 * TRHIP_ERR_INVALID, in this order, the parameter block before any handle: params NULL; tau not > 0 (+Inf is allowed: no extra sample where
 * E is finite); eps not finite or < 0; pilot + max_extra > 2^24; flags != 0; reserved != 0; then a null pointer; a zero dimension or 2^31
 * sample pixels.  The _device variant takes DEVICE pointers for mv, out_counts and out_total and allocates nothing.
 * trhip_sample_map_default_params needs no context and no GPU. */
typedef struct {
    float tau;          /* target relative standard error of a pixel's mean luminance; default 0.25 */
    float eps;          /* added to |m|: keeps black pixels from asking for samples; default 0.01 */
    uint32_t pilot;     /* samples per pixel of the frame mv came from; default 8 */
    uint32_t max_extra; /* cap of a count; default 56 */
    uint32_t flags;     /* 0 */
    uint32_t reserved;  /* 0 */
} trhip_sample_map_params;         /* 24 bytes */
int trhip_sample_map_default_params(trhip_sample_map_params* params);
int trhip_sample_map(trhip_ctx* ctx, const float* mv, uint32_t sb_width, uint32_t sb_height, const trhip_sample_map_params* params, uint32_t* out_counts, uint64_t* out_total);
int trhip_sample_map_device(trhip_ctx* ctx, const void* d_mv, uint32_t sb_width, uint32_t sb_height, const trhip_sample_map_params* params, void* d_out_counts, void* d_out_total);

/* ---- first-hit feature buffers (since ABI 3001, added without a version change: nothing existing moved) -------------------
 * What a denoiser, a compositor, an object picker or an edge-aware upscaler wants beside the beauty frame: for every camera
 * sample of a frame the closest hit of its camera ray — depth, position, geometric and shading normal, base colour, primitive
 * and material id — and the same values filtered onto the film.  The reference has no such output; the entry points below are
 * this library's.  The camera samples are exactly those of the path renderer for the same (sensor, spp, seed, sample_offset):
 * same stream keys, same get_camera_sample dimensions (sampler/sampler.jl:135-139), same generate_ray (camera/perspective.jl:85-114).
 * Every camera ray is traced once, through the closest-hit walk the scene's commit selected (so the hit is the reference's
 * intersect!(bvh, ray)); there are no bounces, no shadow rays and no BSDF: lights are ignored (a scene without any is fine) and
 * primitives without a material are accepted.
 *
 * trhip_aov_sample: one camera sample, 80 bytes = five 16-byte words, 16-byte aligned:
 *   offset  0  t, prim, b1, b2      exactly the trhip_hit of the camera ray (+Inf, -1, 0, 0 on a miss)
 *   offset 16  p[3], material       hit position as the hit-geometry entry point gives it; material = the id the primitive was added
 *                                   with (int32), -1 on a miss and for a primitive without a material
 *   offset 32  n[3], pad0           geometric normal, then a zero word
 *   offset 48  ns[3], pad1          shading normal, then a zero word
 *   offset 64  albedo[3], pad2      base colour, then a zero word
 * On a miss everything but t, prim and material is zero.  (Seventeen 32-bit values do not fit four 16-byte words: the record is five.)
 * Base colour is a DEFINITION OF THIS LIBRARY (the reference has none): the constant texture a material's main lobe is built from,
 * clamped as materials/material.jl clamps it before building the BSDF (clamp(spectrum), spectrum.jl:34-38: to [0, +Inf)) —
 *   TRHIP_MATTE Kd, TRHIP_MIRROR Kr, TRHIP_PLASTIC Kd, TRHIP_GLASS Kt unless it is black after the clamp, then Kr; no material: zero.
 * Records are indexed like the per-sample radiance: [s * n_sample_pixels + (y - sb.min.y) * sb_width + (x - sb.min.x)].
 *
 * out_planes: (crop height) * (crop width) * 3 float4 in film.pixels (y, x) order, plane-minor ([y][x][plane][4]):
 *   plane 0 = (sum w * albedo.rgb, sum w over ALL samples)       — its .w is bit for bit the filter_weight_sum of the path renderer
 *   plane 1 = (sum w * ns.xyz,     sum w over HITTING samples)
 *   plane 2 = (sum w * p.xyz,      sum w * t)
 * w is the film's own weight of the (sample, pixel) pair (add_sample!'s table lookup, film.jl:134-164), samples reach a pixel in the film
 * pass's order (tile k, sample pixel, sample index; one partial sum per tile as merge_film_tile! adds them, film.jl:182-193), only hitting
 * samples enter the sums (except plane 0's weight).  The sums are NOT normalised and no colour conversion is applied: the host divides
 * (the Lanczos lobes are negative, so what a ratio means is the caller's business).  The planes are additive over sample_offset shards:
 * the film all-reduce over 3 * n_pixels "pixels" sums them across the ranks of a multi-GPU job.
 * Either output may be NULL (both: TRHIP_ERR_INVALID).  A frame whose per-sample buffers (152 bytes per camera sample) do not fit in free
 * HBM is refused with TRHIP_ERR_UNSUPPORTED: there are no bands here.  The call fills trhip_stats: camera_samples, closest_rays,
 * fallback_rays, traversal, ms_raygen / ms_trace_closest / ms_fallback / ms_shade (the resolve kernel) / ms_film (the gather) and the launch counts.
 * The _device variant takes DEVICE pointers for both outputs. */
typedef struct {
    float t;
    int32_t prim;
    float b1, b2;
    float p[3];
    int32_t material;
    float n[3];
    uint32_t pad0;
    float ns[3];
    uint32_t pad1;
    float albedo[3];
    uint32_t pad2;
} trhip_aov_sample;
int trhip_render_aov(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                     float* out_planes, trhip_aov_sample* out_samples, trhip_stats* stats);
int trhip_render_aov_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                            void* d_out_planes, void* d_out_samples, trhip_stats* stats);

/* ---- ambient occlusion (since ABI 3001, added without a version change: nothing existing moved) ------------------------------
 * The picture of bare geometry: no lights, no BSDF, primitives without a material accepted (pbrt's `ao` integrator; the reference
 * has none, the definition below is this library's; docs/design/13-ao.md).  The camera samples are exactly those of
 * trhip_render_path / trhip_render_aov for the same (sensor, spp, seed, sample_offset).  For a camera sample with stream key `key`:
 *   1. The camera ray goes through the scene's closest-hit walk, as in trhip_render_aov.
 *        miss: L = (background, background, background);   a hit whose interaction cannot be rebuilt: L = 0.
 *   2. Otherwise, with p, ns of the hit (the hit-geometry entry point's values) and wo = -d:
 *        nf = face_forward(ns, wo);  coordinate_system(nf, s, t)                                      (Trace.jl:170, :139-146)
 *        u  = (ts_uniform(key, ts_vertex_dim(0, TS_V_BSDF_U0)), ts_uniform(key, ts_vertex_dim(0, TS_V_BSDF_U1)))
 *        wl = cosine_sample_hemisphere(u)                                                             (Trace.jl:48-73, sin / cos of trace_detmath.h)
 *        wi = (s * wl.x + t * wl.y) + nf * wl.z                      per component, in that order
 *        the occlusion ray is spawn_ray(si, wi) (Trace.jl:206-211) with a finite reach: o = p + 1e-6f * wi, d = wi, t_max = max_distance,
 *        time = the camera ray's (scenes are static: it acts on nothing)
 *   3. occluded = intersect_p(bvh, ray): the scene's any-hit walk with the ray's own t_max.  max_distance = +Inf is allowed, and the default.
 *   4. v = occluded ? 0 : 1 (the cosine pdf cancels cos / pi).  L = (v, v, v); with TRHIP_AO_ALBEDO, L = v * base colour (trhip_aov_sample's
 *      definition; a primitive without a material gives 0).
 *   5. The per-sample L goes through the path renderer's film pass unchanged (NaN rule, rgb_to_xyz, weights, tile order).
 * Hence out_xyzw is bit for bit what trhip_film_accumulate makes of the same samples, its .w is the path frame's filter_weight_sum (so the
 * film goes into trhip_denoise with the planes of trhip_render_aov), films are additive over sample_offset shards (a multi-GPU job uses the
 * film reduce), and ONE occlusion ray is traced per camera sample: quality comes from spp.  trhip_last_sample_radiance returns this call's L.
 * Lights are ignored; a scene without any is fine.  TRHIP_ERR_INVALID: a null pointer, an uncommitted scene, spp == 0, max_distance NaN or
 * <= 0, background not finite or negative, unknown flag bits, reserved != 0 (the parameter block is checked first, before any handle).
 * A frame whose per-sample buffers do not fit in free HBM is refused with TRHIP_ERR_UNSUPPORTED: there are no bands here.
 * trhip_stats: camera_samples, closest_rays, shadow_rays (the occlusion rays: one per hit), fallback_rays, traversal, ms_raygen /
 * ms_trace_closest / ms_fallback / ms_shade (the spawn kernel) / ms_trace_any / ms_film and the launch counts, n_batches = 1,
 * max_depth_reached = 1.  The _device variant takes a DEVICE pointer for the film.  trhip_ao_default_params needs no context and no GPU. */
#define TRHIP_AO_ALBEDO 1u /* L = v * base colour instead of (v, v, v) */
typedef struct {
    float max_distance;       /* reach of the occlusion rays: > 0 or +Inf */
    float background;         /* radiance of a camera ray that misses: finite, >= 0 */
    uint32_t flags;           /* bit 0: TRHIP_AO_ALBEDO */
    uint32_t reserved;        /* 0 */
} trhip_ao_params;            /* 16 bytes */
int trhip_ao_default_params(trhip_ao_params* out); /* {+Inf, 0, 0, 0} */
int trhip_render_ao(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                    const trhip_ao_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_ao_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                           const trhip_ao_params* params, void* d_out_xyzw, trhip_stats* stats);

/* ---- environment map and sky-lit frames (since ABI 3001, added without a version change: nothing existing moved) ---------------
 * An environment E(w): the radiance that arrives from direction w.  It is an OCTAHEDRAL map of n x n RGB texels, chosen because its
 * lookup is plain arithmetic (no atan2, no acos) and therefore reproducible bit for bit; docs/design/25-sky.md holds the
 * specification.  The reference has no environment light (lights/light.jl:41 returns 0 for an escaping ray): this is the library's own.
 *   rgb            n * n * 3 floats, row j, column i: texel (i, j) at rgb[3 * (j * n + i)].  Texel centre (i, j) lies at the point
 *                  (px, py) = ((i + 0.5) / n * 2 - 1, (j + 0.5) / n * 2 - 1) of the octahedral square.
 *   world_to_env   9 floats, row-major R[3 * r + c]: the lookup multiplies every direction by it, the identity included.
 * The handle keeps (n + 2)^2 float4 texels in HBM: the map and a one-texel gutter filled at creation.  The gutter texel (i, j) with i outside
 * [0, n) is the interior texel (clamp(i), n - 1 - j); with j outside, (n - 1 - i, clamp(j)); a corner applies one rule after the other (the
 * octahedral edge wrap), so the lookup needs no clamp and no branch at the border.
 * The lookup, one Float32 operation per line, in this order, no contraction, `/` correctly rounded:
 *   e_r = (R[r][0] * w.x + R[r][1] * w.y) + R[r][2] * w.z                      r = 0, 1, 2
 *   s = (|e.x| + |e.y|) + |e.z|;   !(s > 0) or s not finite: E = (+0, +0, +0)   (zero, NaN and Inf directions)
 *   px = e.x / s,  py = e.y / s
 *   e.z < 0:  qx = (1 - |py|) * sgn(px),  qy = (1 - |px|) * sgn(py),  (px, py) = (qx, qy)       sgn(v) = v < 0 ? -1 : 1
 *   fx = (px * 0.5 + 0.5) * n - 0.5,  fy likewise                              (three operations each)
 *   x0 = floor(fx),  tx = fx - x0,  y0 = floor(fy),  ty = fy - y0;  x0, y0 lie in [-1, n - 1] and are clamped there as integers
 *   per channel: lerp(lerp(T[x0, y0], T[x0 + 1, y0], tx), lerp(T[x0, y0 + 1], T[x0 + 1, y0 + 1], tx), ty),  lerp(a, b, t) = a + t * (b - a)
 * (a == b returns a exactly: a constant map evaluates to its constant in every bit).
 * TRHIP_ERR_INVALID: a null pointer; n == 0 or n > 4096; a texel that is not finite or is negative (the contributions of a sky frame's
 * any-hit queue carry no poison bits and must be finite); a matrix entry that is not finite — all checked before the context is looked at.
 * trhip_env_eval evaluates `count` directions (count * 3 floats) on the device into count * 3 floats: the lookup on its own, for tests
 * and tools.  An environment belongs to the context it was created with; free it before that context is shut down. */
typedef struct trhip_env trhip_env;
int trhip_env_create(trhip_ctx* ctx, const float* rgb, uint32_t n, const float world_to_env[9], trhip_env** out);
void trhip_env_free(trhip_env* env);
int trhip_env_size(const trhip_env* env, uint32_t* n);
int trhip_env_eval(trhip_ctx* ctx, const trhip_env* env, const float* dirs3, uint64_t count, float* out_rgb3);

/* A sky-lit frame: trhip_render_ao (above) with two substitutions.  The camera samples, the closest-hit walk, the occlusion ray (o, d,
 * t_max, the 1e-6f offset, check_direction) and the any-hit walk are that frame's, step for step; then
 *   the contribution of an unoccluded occlusion ray is c = E(wi) * scale per channel — times the base colour, per channel, under
 *     TRHIP_SKY_ALBEDO (zero for a primitive without a material) — where trhip_render_ao has 1 or the base colour;
 *   a camera ray that misses returns L = E(d) * scale for its direction d, or 0 under TRHIP_SKY_HIDE_BACKGROUND, where trhip_render_ao
 *     has its background.
 * With cosine-distributed wi the pdf cancels cos / pi, so c is the unbiased one-sample estimate of direct diffuse lighting under the
 * environment.  The per-sample L goes through the path renderer's film pass; trhip_last_sample_radiance returns it.  Statistics are
 * trhip_render_ao's; there are no bands (TRHIP_ERR_UNSUPPORTED when the per-sample buffers do not fit in free HBM).
 * TRHIP_ERR_INVALID: trhip_render_ao's refusals in its order (the parameter block first, before any handle), with `scale` not finite or
 * negative in the place of its background; then a null env, an env of another context, and a scale that takes the map's largest texel
 * to +Inf.  trhip_sky_default_params needs no context and no GPU. */
#define TRHIP_SKY_ALBEDO 1u          /* c = E(wi) * scale * base colour */
#define TRHIP_SKY_HIDE_BACKGROUND 2u /* a camera ray that misses returns 0 */
typedef struct {
    float max_distance;       /* reach of the occlusion rays: > 0 or +Inf */
    float scale;              /* multiplies every lookup: finite, >= 0 */
    uint32_t flags;           /* TRHIP_SKY_ALBEDO | TRHIP_SKY_HIDE_BACKGROUND */
    uint32_t reserved;        /* 0 */
} trhip_sky_params;           /* 16 bytes */
int trhip_sky_default_params(trhip_sky_params* out); /* {+Inf, 1, 0, 0} */
int trhip_render_sky(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                     const trhip_env* env, const trhip_sky_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_sky_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                            const trhip_env* env, const trhip_sky_params* params, void* d_out_xyzw, trhip_stats* stats);

/* ---- environment light in path frames (since ABI 3001, added without a version change: nothing existing moved) -----------------
 * trhip_render_path with one change (docs/design/26-path-env.md): where the closest-hit walk finds nothing at depth d (1 <= d <=
 * max_depth) the path records an ESCAPE — the depth d, its throughput beta at that moment and the ray's direction dir — and ends, as it
 * ends in trhip_render_path.  The sample's radiance is
 *   L' = L + beta * (E(dir) * scale)          c = E * scale, t = beta * c, L' = L + t per channel: one Float32 operation each, no contraction
 * where L is exactly what trhip_render_path computes for that sample and E the lookup above; the escape is the last addend in depth order.
 * Under TRHIP_PATH_ENV_HIDE_BACKGROUND a depth-1 escape adds nothing (its record is still written).  A path escapes at most once; a path
 * that is absorbed, loses Russian roulette or is cut at max_depth has no escape (depth 0).  A non-finite beta gives what IEEE gives; the
 * film pass and trhip_last_sample_radiance apply the NaN rule to L' as they apply it to L.  No importance sampling of the map: with BSDF
 * sampling beta * E(dir) is an unbiased estimate, and for specular lobes the only one.
 * The frame is the classic per-depth wavefront: options "streaming" and "band_tile_rows" are ignored, "pipelines", "overlap" and
 * "batch_paths" hold.  There are no bands: TRHIP_ERR_UNSUPPORTED when the per-sample buffers (64 bytes per camera sample beside the film
 * pass's own) do not fit in half of free HBM.  Statistics are trhip_render_path's.
 * TRHIP_ERR_INVALID, in this order: the parameter block (NULL; scale not finite or negative; unknown flag bits; reserved), checked before
 * any handle is looked at; trhip_render_path's refusals in its order; a null env; an env of another context; a scale that takes the
 * map's largest texel to +Inf.  trhip_path_env_default_params needs no context and no GPU.
 *
 * trhip_last_escapes: after a path-env frame (TRHIP_ERR_INVALID after anything else), 8 floats per camera sample — beta.xyz, the escape
 * depth as a number (0 = none), dir.xyz, 0 — indexed like trhip_last_sample_radiance; n_floats must be 8 times its sample count.
 *
 * trhip_path_env_relight: folds the frame's retained radiance and escape records with ANOTHER environment and / or other parameters, then
 * runs the film pass exactly as the frame ran it: film and trhip_last_sample_radiance equal a fresh trhip_render_path_env with those
 * arguments bit for bit, without a single ray.  Valid only while the context's last frame is a path-env frame: after any other render,
 * film or image-pass call it returns TRHIP_ERR_INVALID.  Refusals otherwise as the frame's: parameter block, null arguments, no such
 * frame, then the environment's three. */
#define TRHIP_PATH_ENV_HIDE_BACKGROUND 1u /* a depth-1 escape (a camera ray that misses) adds nothing */
typedef struct {
    float scale;              /* multiplies every lookup: finite, >= 0 */
    uint32_t flags;           /* TRHIP_PATH_ENV_HIDE_BACKGROUND */
    uint32_t reserved[2];     /* 0 */
} trhip_path_env_params;      /* 16 bytes */
int trhip_path_env_default_params(trhip_path_env_params* out); /* {1, 0, {0, 0}} */
int trhip_render_path_env(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                          const trhip_env* env, const trhip_path_env_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_path_env_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                                 const trhip_env* env, const trhip_path_env_params* params, void* d_out_xyzw, trhip_stats* stats);
int trhip_last_escapes(trhip_ctx* ctx, float* out8, uint64_t n_floats);
int trhip_path_env_relight(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* params, float* out_xyzw);
int trhip_path_env_relight_device(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* params, void* d_out_xyzw);

/* ---- importance sampling of the environment map (since ABI 3001, added without a version change: nothing existing moved) ---------
 * docs/design/27-sky-importance.md holds the specification.  trhip_env_make_sampler builds, once and on the host in Float64, a
 * piecewise-constant distribution over the map's n x n cells (the channel sum of the interpolated map integrated over each cell, times
 * the solid angle per unit area of the octahedral square at the cell's centre) and keeps its tables, (n + 1)^2 floats, with the handle;
 * it is idempotent, and trhip_env_free frees the tables.  TRHIP_ERR_INVALID, in this order: a null argument; an env of another context;
 * a world_to_env that is not orthonormal (max |R R^T - I| > 1e-5: sampling needs R^-1 = R^T); a map whose weights are all zero.
 * trhip_env_sample maps `count` points u = (u0, u1) of [0, 1)^2 (count * 2 floats) to unit directions (count * 3 floats), distributed
 * like the table; trhip_env_pdf returns the density of `count` directions with respect to solid angle (0 where the lookup has no
 * answer).  Both run on the device and are specified bit for bit; their refusals are trhip_env_eval's, plus an env without a sampler.
 *
 * trhip_render_sky_is is trhip_render_sky with one substitution per hit: with probability `mix` the occlusion ray's direction is drawn
 * from the map's distribution instead of the cosine lobe, and the contribution is that of the one-sample mixture estimator,
 *   c = (E(wi) * scale) * g,   g = pc / ((1 - mix) pc + mix pe),   pc = cos / pi,   pe = trhip_env_pdf(wi),
 * unbiased wherever cos > 0 and never larger than E * scale / (1 - mix).  Everything else — camera samples, walks, the miss term, the
 * flags, the film pass, statistics, trhip_last_sample_radiance — is trhip_render_sky's.  TRHIP_ERR_INVALID: trhip_render_sky's refusals
 * in its order, with `mix` outside (0, 1) or not finite after `reserved` (still before any handle is looked at); then an env without a
 * sampler, and a scale for which (largest texel) * scale / (1 - mix) is not finite.  trhip_sky_is_default_params needs no context. */
int trhip_env_make_sampler(trhip_ctx* ctx, trhip_env* env);
int trhip_env_sample(trhip_ctx* ctx, const trhip_env* env, const float* u2, uint64_t count, float* out_dir3);
int trhip_env_pdf(trhip_ctx* ctx, const trhip_env* env, const float* dirs3, uint64_t count, float* out_pdf);
typedef struct {
    float max_distance;       /* reach of the occlusion rays: > 0 or +Inf */
    float scale;              /* multiplies every lookup: finite, >= 0 */
    float mix;                /* probability of drawing the direction from the map: in (0, 1) */
    uint32_t flags;           /* TRHIP_SKY_ALBEDO | TRHIP_SKY_HIDE_BACKGROUND */
    uint32_t reserved[4];     /* 0 */
} trhip_sky_is_params;        /* 32 bytes */
int trhip_sky_is_default_params(trhip_sky_is_params* out); /* {+Inf, 1, 0.5, 0, {0, 0, 0, 0}} */
int trhip_render_sky_is(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                        const trhip_env* env, const trhip_sky_is_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_sky_is_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                               const trhip_env* env, const trhip_sky_is_params* params, void* d_out_xyzw, trhip_stats* stats);

/* ---- next-event estimation of the environment map in path frames (since ABI 3001, added without a version change: nothing existing moved)
 * trhip_render_path_env with two changes (docs/design/28-path-nee.md holds the specification, step by step):
 *  1. at every vertex whose BSDF has a non-specular lobe — the last one, at max_depth, included — one shadow ray estimates the map's direct
 *     light with the one-sample mixture of BSDF sampling and map sampling: with probability `mix` the direction wi is trhip_env_sample's
 *     (from the vertex's TS_V_LIGHT_U0 / U1 numbers), otherwise the non-specular lobes' sample (from TS_V_SCATTER_U0 / U1), and where
 *     the ray reaches nothing the sample gains
 *       beta * ((f(wo, wi) |wi . n|) * (E(wi) * scale) / ((1 - mix) pdf_bsdf(wi) + mix trhip_env_pdf(wi)))
 *     after the vertex's point-light term.  The path itself — its rays, its throughput, its Russian roulette — is trhip_render_path's
 *     in every bit: the continuation keeps TS_V_BSDF_U0 / U1 to itself;
 *  2. an escape that follows such a vertex no longer counts (its light is already estimated): an escape at depth d contributes as in
 *     trhip_render_path_env if and only if d == 1 (without TRHIP_PATH_ENV_HIDE_BACKGROUND) or vertex d - 1 had specular lobes only.
 * With scale == 0 the frame is trhip_render_path, and in a scene without a non-specular material trhip_render_path_env, bit for bit.
 * trhip_last_escapes works after the frame: a suppressed escape still leaves its record, with the 8th float 1 in place of 0.
 * trhip_path_env_relight refuses it (TRHIP_ERR_INVALID): the base radiance contains the map.  Options, bands and statistics as
 * trhip_render_path_env; shadow_rays counts the point-light rays and the NEE rays.
 * Refusals, in this order: the parameter block (NULL; scale; unknown flag bits; reserved; mix not finite or outside (0, 1)), before any
 * handle is looked at; trhip_render_path_env's in its order; an env without a sampler (trhip_env_make_sampler); TRHIP_ERR_UNSUPPORTED
 * for a scene with a material whose lobe set mixes specular and non-specular lobes (trhip_scene_add_material builds none), and for a
 * frame whose per-sample buffers and NEE shadow queues do not fit in half of free HBM.  trhip_path_nee_default_params needs no context. */
typedef struct {
    float scale;              /* multiplies every lookup: finite, >= 0 */
    float mix;                /* probability of drawing the direction from the map: in (0, 1) */
    uint32_t flags;           /* TRHIP_PATH_ENV_HIDE_BACKGROUND */
    uint32_t reserved[5];     /* 0 */
} trhip_path_nee_params;      /* 32 bytes */
int trhip_path_nee_default_params(trhip_path_nee_params* out); /* {1, 0.5, 0, {0, 0, 0, 0, 0}} */
int trhip_render_path_env_nee(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                              const trhip_env* env, const trhip_path_nee_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_path_env_nee_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                                     const trhip_env* env, const trhip_path_nee_params* params, void* d_out_xyzw, trhip_stats* stats);

/* ---- area lights in path frames: emissive triangles (since ABI 3001, added without a version change: nothing existing moved)
 * docs/design/29-path-emit.md holds the specification, step by step.
 *
 * An emitter set is made from a committed scene: every triangle whose material id is listed emits that material's radiance Le, on both sides.  Emitters are ordered by
 * canonical primitive slot, ascending.  The set belongs to the scene's committed geometry (trhip_scene_geometry_id) and serves every relit view of it.  Its sampling table
 * is built once on the host in Float64: weight_j = area_j * (Le.r + Le.g + Le.b), a cdf of n + 1 Float32 values; pick(xi) is the largest j with cdf[j] <= xi, the point
 * s = sqrt(u0), b0 = 1 - s, b1 = u1 s, b2 = (1 - b0) - b1, y = (b0 p0 + b1 p1) + b2 p2, and the area density P_j / A_j with P_j = cdf[j + 1] - cdf[j].
 * trhip_emitters_create refuses, in this order: null arguments or n_materials == 0; a radiance component that is not finite or is negative (before any handle is looked
 * at); a scene that is not committed or belongs to another context; an unknown or repeated material id; a listed material carried by a sphere (TRHIP_ERR_UNSUPPORTED); no
 * triangle with positive weight; more than 2^20 emissive triangles (TRHIP_ERR_UNSUPPORTED).
 * trhip_emitters_sample runs pick and point on the device for `count` triples (xi, u0, u1): the emitter's index, the point and the area density. */
typedef struct trhip_emitters trhip_emitters;
int trhip_emitters_create(trhip_ctx* ctx, const trhip_scene* scene, const uint32_t* material_ids, const float* radiance_rgb3, uint32_t n_materials, trhip_emitters** out);
void trhip_emitters_free(trhip_emitters* em);
int trhip_emitters_size(const trhip_emitters* em, uint32_t* n_triangles);
int trhip_emitters_sample(trhip_ctx* ctx, const trhip_emitters* em, const float* u3, uint64_t count, uint32_t* out_index, float* out_point3, float* out_pdf_area);

/* trhip_render_path_emit: trhip_render_path in which the emitters shine.  At a hit at depth d (vertex v = d - 1):
 *  1. where the hit triangle's material emits, and d == 1 or vertex d - 1 had specular lobes only or TRHIP_PATH_EMIT_HITS_ONLY is set, the sample's emitted sum gains
 *     beta * (Le * scale);
 *  2. the path continues exactly as in trhip_render_path — its rays, its throughput, its point-light term, its Russian roulette — in every bit;
 *  3. without HITS_ONLY, at every vertex whose BSDF has a non-specular lobe — the last one, at max_depth, included — one shadow ray estimates the emitters' direct light:
 *     (xi, u0, u1) = ts_uniform(key, TS_DIM_EMIT_BASE + 3 v + {0, 1, 2}), j = pick(xi), y = point_j(u0, u1), wi = (y - p) / dist, and where nothing lies within
 *     dist * 0.999 the sample gains  beta * ((f(wo, wi) |wi . n|) * (Le_j * scale) / ((P_j / A_j) dist^2 / |n_j . wi|))  after the vertex's point-light term.
 * Per sample the radiance is L + Lh (the emitted sum, added to in depth order), then the NaN rule and the film pass.  With scale == 0 the frame is trhip_render_path bit
 * for bit wherever the throughput stays finite; with HITS_ONLY it is plain path tracing, the unbiased reference estimator.
 * trhip_last_emitted: 4 floats per camera sample — Lh.rgb and the number of counted hits —, indexed like trhip_last_sample_radiance; valid only after an emit frame.
 * Options and statistics as trhip_render_path_env (no bands, no streaming); shadow_rays counts the point-light rays and the emitter rays.
 * Refusals, in this order: the parameter block (NULL; scale not finite or negative; unknown flag bits; reserved), before any handle is looked at; trhip_render_path's in
 * its order; null emitters or emitters of another context; emitters of another geometry than the scene's; TRHIP_ERR_UNSUPPORTED for a scene with a material whose lobe set
 * mixes specular and non-specular lobes, and for a frame whose per-sample buffers and shadow queues do not fit in half of free HBM.
 * trhip_path_emit_default_params needs no context. */
#define TRHIP_PATH_EMIT_HITS_ONLY 1u /* no next-event estimation; every hit on an emitter counts */
typedef struct {
    float scale;              /* multiplies every Le: finite, >= 0 */
    uint32_t flags;           /* TRHIP_PATH_EMIT_HITS_ONLY */
    uint32_t reserved[6];     /* 0 */
} trhip_path_emit_params;     /* 32 bytes */
int trhip_path_emit_default_params(trhip_path_emit_params* out); /* {1, 0, {0, 0, 0, 0, 0, 0}} */
int trhip_render_path_emit(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                           const trhip_emitters* emitters, const trhip_path_emit_params* params, float* out_xyzw, trhip_stats* stats);
int trhip_render_path_emit_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                                  const trhip_emitters* emitters, const trhip_path_emit_params* params, void* d_out_xyzw, trhip_stats* stats);
int trhip_last_emitted(trhip_ctx* ctx, float* out4, uint64_t n_floats);

/* ---- edge-avoiding denoiser for path / Whitted films (since ABI 3001, added without a version change: nothing existing moved) ----
 * An à-trous wavelet filter after Dammertz et al. 2010 ("Edge-Avoiding À-Trous Wavelet Transform for fast Global Illumination
 * Filtering") on the film state of a path or Whitted render, guided by the three planes of trhip_render_aov for the same sensor,
 * spp, seed and sample offset.  The reference has no such pass; the arithmetic is this library's and is specified, operation by
 * operation, in docs/design/12-denoise.md: every step is one Float32 operation in a fixed order, `/` and sqrt correctly rounded, no
 * transcendental function, so the output is reproducible bit for bit.  The edge-stopping function is Tukey's biweight,
 * g(x) = x < 1 ? (1 - x*x)^2 : 0, in place of exp: a neighbour across a hard edge weighs exactly 0.
 *   xyzw      height * width float4, exactly what trhip_render_path / trhip_render_whitted wrote
 *   planes    height * width * 3 float4, exactly what trhip_render_aov wrote
 *   out_xyzw  the layout of xyzw; may be xyzw itself
 * A pixel is a SURFACE pixel when its filter weight, its total plane weight and its hit weight are positive, the hit weight is at
 * least min_coverage times the total weight, and its normal, position and colour are finite.  Only surface pixels are filtered and
 * only surface pixels are read as neighbours; every other pixel (a miss — path and Whitted frames have no environment term —, a silhouette
 * pixel under min_coverage, a NaN) is returned with its input bits.  The .w lane (the filter weight sum) is always returned as given.
 * iterations = 0 copies.  The step of iteration i is 2^i pixels and its colour sigma is sigma_colour * 2^-i.
 * TRHIP_ERR_INVALID: a null pointer, a zero dimension, iterations > 6, a sigma or albedo_floor that is not finite and > 0,
 * min_coverage outside [0, 1], unknown flag bits, reserved != 0.  TRHIP_ERR_UNSUPPORTED: the working set (80 bytes per pixel) does
 * not fit in free HBM; the film is not split into bands.  stats (may be NULL): ms_total, ms_film / launches_film over all of the
 * call's kernels, and their parts in ms_sub / launches_sub: [0] prepare, [1] the iterations, [2] finish.  The _device variant takes DEVICE pointers for the three images.
 * trhip_denoise_default_params needs no context and no GPU. */
#define TRHIP_DENOISE_DEMODULATE 1u /* divide by the base colour (clamped below by albedo_floor) before filtering, multiply after */
typedef struct {
    uint32_t iterations;      /* 0..6; 0 = copy */
    uint32_t flags;           /* bit 0: TRHIP_DENOISE_DEMODULATE */
    float sigma_colour;       /* on |dY| of the (demodulated) linear RGB; halved every iteration */
    float sigma_normal;       /* on 1 - n_p . n_q */
    float sigma_plane;        /* on |n_p . (p_q - p_p)|, world units */
    float albedo_floor;       /* lower clamp of the base colour used for demodulation */
    float min_coverage;       /* a pixel is a surface pixel when hit weight >= min_coverage * total weight */
    uint32_t reserved;        /* 0 */
} trhip_denoise_params;       /* 32 bytes */
int trhip_denoise_default_params(trhip_denoise_params* out);
int trhip_denoise(trhip_ctx* ctx, const float* xyzw, const float* planes, uint32_t width, uint32_t height, const trhip_denoise_params* params,
                  float* out_xyzw, trhip_stats* stats);
int trhip_denoise_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, uint32_t width, uint32_t height, const trhip_denoise_params* params,
                         void* d_out_xyzw, trhip_stats* stats);

/* ---- temporal reprojection for moving-camera previews (since ABI 3001, added without a version change: nothing existing moved) ----
 * The first step of SVGF (Schied et al. 2017, "Spatiotemporal Variance-Guided Filtering", section 4.1): the previous frame's accumulated
 * colour is fetched through the PREVIOUS camera at the world position of each pixel's surface, validated against the feature planes, and
 * blended with the new frame; trhip_denoise then filters the result with the current frame's planes.  Image-space: no scene, no traversal.
 * The arithmetic is specified, operation by operation, in docs/design/14-temporal.md and is bit-reproducible like the denoiser's.
 *
 * trhip_sensor_world_to_pixel: out12 = M, a row-major 3 x 4 matrix.  For a world point p, h_i = ((M[i][0]*p.x + M[i][1]*p.y) + M[i][2]*p.z) +
 * M[i][3]; (h.x / h.z, h.y / h.z) is p's position in film-ARRAY pixel coordinates — 0-based, integers at pixel centres, [y][x] as in out_xyzw —
 * valid iff h.z > 0 (p in front of the camera).  Built in Float64 from raster_to_camera, camera_to_world and crop_min, each entry rounded to
 * Float32 once; depth of field is ignored (the lens centre is the projection centre).  A singular matrix: TRHIP_ERR_INVALID.  No context, no GPU.
 *
 * trhip_temporal:
 *   xyzw, planes, out_xyzw   as in trhip_denoise; out_xyzw may be xyzw itself
 *   history, out_history     height * width * 3 float4, plane-minor like planes: (c.rgb, N) accumulated linear RGB and history length,
 *                            (n.xyz, 1 if surface else 0), (p.xyz, 0).  history may be NULL (first frame, or after a change of lights or film size)
 * Per pixel: a pixel that is no surface pixel (trhip_denoise's rule, min_coverage) is returned with its input bits and a zero history record.
 * A surface pixel at world position p is projected with prev_world_to_pixel; the four history pixels around that position are bilinear taps, a
 * tap counting when it lies inside the image, was a surface pixel with N > 0, 1 - n.n_q < sigma_normal and |n.(p_q - p)| < sigma_plane.  With
 * c_h, N_h the weighted means over the counting taps: N' = min(N_h + 1, max_history), c' = c_h + (c - c_h) / N'; without any (or h.z <= 0, a
 * position that is not finite or beyond 2^20, a result that is not finite): c' = c, N' = 1.  out_xyzw = (rgb_to_xyz(c') * w, w): the .w lane
 * is returned as given, so the output goes into trhip_denoise, film.set_xyzw and save.  Scenes are static (rigid bodies that move between frames:
 * trhip_temporal_motion, below); lighting changes are NOT detected: pass history = NULL after one.
 * TRHIP_ERR_INVALID: params NULL, an entry of prev_world_to_pixel not finite, max_history not finite or < 1, flags != 0, a sigma not finite
 * and > 0, min_coverage outside [0, 1], reserved != 0 (the parameter block is checked first, before any handle); then a null pointer (history
 * excepted), a zero dimension, out_history overlapping history, planes, xyzw or out_xyzw.  TRHIP_ERR_UNSUPPORTED: the host variant's device
 * copies (160 bytes per pixel) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes
 * DEVICE pointers for the five images.  trhip_temporal_default_params needs no context and no GPU; it leaves prev_world_to_pixel zero (no
 * history is found through it). */
typedef struct {
    float prev_world_to_pixel[12]; /* trhip_sensor_world_to_pixel of the PREVIOUS frame's sensor */
    float max_history;             /* cap of the history length: finite, >= 1 */
    float sigma_normal;            /* a tap is accepted when 1 - n.n_q   < sigma_normal */
    float sigma_plane;             /* ... and |n.(p_q - p)| < sigma_plane, world units */
    float min_coverage;            /* the denoiser's surface-pixel rule, [0, 1] */
    uint32_t flags;                /* 0 */
    uint32_t reserved;             /* 0 */
} trhip_temporal_params;           /* 72 bytes */
int trhip_sensor_world_to_pixel(const trhip_sensor* sensor, float out12[12]);
int trhip_temporal_default_params(trhip_temporal_params* out);
int trhip_temporal(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, uint32_t width, uint32_t height, const trhip_temporal_params* params,
                   float* out_xyzw, float* out_history, trhip_stats* stats);
int trhip_temporal_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, uint32_t width, uint32_t height, const trhip_temporal_params* params,
                          void* d_out_xyzw, void* d_out_history, trhip_stats* stats);

/* ---- variance clipping of the reprojected history (since ABI 3001, added without a version change: nothing existing moved) ----
 * trhip_temporal with the standard remedy for stale history (Salvi 2016, "An excursion in temporal supersampling"): before the blend, the
 * reprojected history colour is confined to mean +- clip_gamma * sd of the NEW frame's colours in a window around the pixel.  A history that
 * no longer fits the frame — old lighting after trhip_scene_relight, blur and view-dependent shading carried along — is cut back in one frame
 * instead of fading at 1 - 1/max_history per frame.  Specified operation by operation in docs/design/15-temporal-clip.md; bit-reproducible.
 *
 * trhip_temporal_clip: the images, the overlap rules and stats as in trhip_temporal.  Per surface pixel with n, p, c: over the window dy = -R..R
 * outer, dx = -R..R inner (R = clip_radius), the centre counts, another position counts when it lies inside the image, is a surface pixel,
 * 1 - n.n_q < base.sigma_normal and |n.(p_q - p)| < base.sigma_plane; over the counting positions m1 += c_q, m2 += c_q * c_q, cnt += 1 per
 * channel, in that order.  mean = m1 / cnt, var = max(m2 / cnt - mean * mean, 0), sd = sqrt(var), lo = mean - gamma * sd, hi = mean + gamma * sd.
 * trhip_temporal's c_h is then replaced by (c_h < lo) ? lo : ((c_h > hi) ? hi : c_h) per channel and everything else, N' included, goes on as
 * there.  Comparisons with NaN are false: clip_gamma = +Inf gives trhip_temporal's result bit for bit.  The history length is not shortened
 * when a clip fires.  out_xyzw may be xyzw: the _device variant then writes through a film held by the context (16 bytes per pixel, one
 * device-to-device copy more), since a window reads its neighbours' film pixels.  The option "temporal_patch" has no effect on this pass.
 * TRHIP_ERR_INVALID: params NULL; trhip_temporal's refusals on base, in its order; clip_gamma NaN or < 0; clip_radius not 1, 2 or 3; flags != 0;
 * reserved != 0 (all of the parameter block is checked first, before any handle); then trhip_temporal's refusals of pointers, sizes and overlaps.
 * TRHIP_ERR_UNSUPPORTED: the host variant's device copies (176 bytes per pixel) do not fit in free HBM.
 * trhip_temporal_clip_default_params needs no context and no GPU: base as trhip_temporal_default_params fills it, clip_gamma = 4 and
 * clip_radius = 3 — of the swept cells that clip (gamma 0.5, 1, 2, 4 x R 1, 2, 3) the one with the lowest geometric mean of the four moving-camera
 * ratios at max_history 8 (profiles/r12/temporal_clip.txt).  On a moving camera no cell beats not clipping; after a change of lights the default
 * leaves 0.28 of the unclipped error in the first frame, gamma = 1 with R = 1 leaves 0.09 and costs 1.46 x the unclipped error on the arcs. */
typedef struct {
    trhip_temporal_params base;    /* as trhip_temporal takes it; base.flags and base.reserved must be 0 */
    float clip_gamma;              /* >= 0 or +Inf; +Inf: trhip_temporal's result bit for bit */
    uint32_t clip_radius;          /* 1, 2 or 3: a window of 3 x 3, 5 x 5 or 7 x 7 pixels */
    uint32_t flags;                /* 0 */
    uint32_t reserved;             /* 0 */
} trhip_temporal_clip_params;      /* 88 bytes */
int trhip_temporal_clip_default_params(trhip_temporal_clip_params* out);
int trhip_temporal_clip(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, uint32_t width, uint32_t height, const trhip_temporal_clip_params* params,
                        float* out_xyzw, float* out_history, trhip_stats* stats);
int trhip_temporal_clip_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, uint32_t width, uint32_t height,
                               const trhip_temporal_clip_params* params, void* d_out_xyzw, void* d_out_history, trhip_stats* stats);

/* ---- luminance moments and a variance plane along the reprojection (since ABI 3001, added without a version change: nothing existing moved) ----
 * The variance estimate of SVGF (Schied et al. 2017, section 4.2), image-space: trhip_temporal with the first two moments of the luminance
 * the denoiser compares carried along the same reprojection, and a spatial estimate where the history is short.  Specified operation by
 * operation in docs/design/16-variance.md; bit-reproducible.
 *
 * trhip_temporal_moments: xyzw, planes, history, out_xyzw, out_history, the overlap rules and stats as in trhip_temporal; out_xyzw and
 * out_history are trhip_temporal's BIT FOR BIT for the same inputs, and the history records are interchangeable with that entry point's.
 *   moments, out_moments   height * width float2 (m1, m2): the accumulated mean of Yd and of Yd * Yd.  moments is NULL exactly when history is
 *   out_variance           height * width float: the variance of the accumulated luminance, >= 0 and finite; 0 where the pixel is no surface pixel
 * Per surface pixel: Yd = to_Y(c / a) with the denoiser's clamped base colour a when flags has TRHIP_DENOISE_DEMODULATE, else to_Y(c), c the new
 * frame's colour.  Over the taps trhip_temporal accepted, with its weights b: s1 += b * m1_q, s2 += b * m2_q.  With sb > 0: m1_h = s1 / sb,
 * m2_h = s2 / sb, m1' = m1_h + (Yd - m1_h) / N', m2' = m2_h + (Yd * Yd - m2_h) / N', vt = max(m2' - m1' * m1', 0); else, or where trhip_temporal
 * falls back to c' = c, or where m1' or m2' is not finite: m1' = Yd, m2' = Yd * Yd and there is no vt.  The spatial estimate vs is taken over
 * trhip_temporal_clip's window at clip_radius 3 — the same order, the same positions count —: S1 += Yd_q, S2 += Yd_q * Yd_q, cnt += 1,
 * mean = S1 / cnt, vs = max(S2 / cnt - mean * mean, 0).  v = vt where there is one and N' < spatial_below is false, else vs;
 * out_variance = v / N' (0 if that is not finite): the variance of a mean of N' frames.  It is NOT the variance of the exponential average the
 * blend becomes at the cap, and it ignores the correlation bilinear resampling puts between neighbours.  history = NULL: every surface pixel
 * gets the spatial estimate.  out_xyzw may be xyzw: the _device variant then writes through a film held by the context, as trhip_temporal_clip.
 * TRHIP_ERR_INVALID, in this order, all on the parameter block before any handle: params NULL; trhip_temporal's refusals on base, in its
 * order; albedo_floor not finite and > 0; spatial_below not finite or < 1; unknown flag bits; reserved != 0.  Then trhip_temporal's refusals of
 * pointers, sizes and overlaps, moments NULL when history is not (or the reverse), a NULL out_moments or out_variance, and out_history,
 * out_moments or out_variance overlapping an input or another output.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (196 bytes
 * per pixel) do not fit in free HBM.  trhip_temporal_moments_default_params needs no context and no GPU. */
typedef struct {
    trhip_temporal_params base;    /* as trhip_temporal takes it; base.flags and base.reserved must be 0 */
    float albedo_floor;            /* the denoiser's; finite, > 0 */
    float spatial_below;           /* N' < spatial_below uses the spatial estimate; finite, >= 1 */
    uint32_t flags;                /* bit 0: TRHIP_DENOISE_DEMODULATE, meaning as in trhip_denoise */
    uint32_t reserved;             /* 0 */
} trhip_temporal_moments_params;   /* 88 bytes */
int trhip_temporal_moments_default_params(trhip_temporal_moments_params* out);
int trhip_temporal_moments(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, const float* moments, uint32_t width, uint32_t height,
                           const trhip_temporal_moments_params* params, float* out_xyzw, float* out_history, float* out_moments, float* out_variance, trhip_stats* stats);
int trhip_temporal_moments_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, const void* d_moments, uint32_t width, uint32_t height,
                                  const trhip_temporal_moments_params* params, void* d_out_xyzw, void* d_out_history, void* d_out_moments, void* d_out_variance,
                                  trhip_stats* stats);

/* ---- variance-guided à-trous filter (since ABI 3001, added without a version change: nothing existing moved) ----
 * trhip_denoise with the colour edge-stop of SVGF (section 4.3): the colour sigma of a pixel is base.sigma_colour times the standard deviation
 * of its luminance, from a variance plane (trhip_temporal_moments') that is filtered along with the colour, plus var_eps.  A pixel with a long
 * history is compared strictly, a pixel disoccluded this frame loosely.  Specified in docs/design/16-variance.md; bit-reproducible.
 *   xyzw, planes, out_xyzw   as in trhip_denoise; out_xyzw may be xyzw itself
 *   variance                 height * width float; read as (v > 0) ? v : 0, so NaN, negatives and -Inf count as 0; +Inf removes the colour
 *                            edge-stop of the pixels whose pre-filter reaches it.  Every output colour is finite whatever the plane holds
 *   out_variance             height * width float or NULL; may be variance itself: the variance of the filtered colour, 0 off surfaces
 * Prepare and Finish are trhip_denoise's.  Iteration i (step 2^i), surface pixel p: gv = the 3 x 3 mean of V_i at unit offsets (weights
 * 0.5 / 0.25 per axis, positions outside the image or off surfaces skipped), sig = base.sigma_colour * sqrt(gv) + var_eps — NOT halved per
 * iteration —; trhip_denoise's taps and weights with wc = g(|Y_q - Y_p| / sig); vsum += (w * w) * V_i(q); V_{i+1}(p) = vsum / (ws * ws), a NaN
 * stored as 0.  With iterations = 1 and a variance plane of 1.0, sig = base.sigma_colour + var_eps and out_xyzw is trhip_denoise's bit for bit.
 * TRHIP_ERR_INVALID, the parameter block first and before any handle: params NULL; trhip_denoise's refusals on base, in its order; var_eps not
 * finite and > 0; flags != 0; reserved != 0; then a null pointer (out_variance excepted), a zero dimension.  TRHIP_ERR_UNSUPPORTED: the
 * working set (88 bytes per pixel; the host variant 68 more) does not fit in free HBM.  stats as trhip_denoise: ms_sub [0] prepare and the
 * variance's seeding, [1] the iterations, [2] finish and the variance's export. */
typedef struct {
    trhip_denoise_params base;     /* base.sigma_colour multiplies the standard deviation; it is NOT halved per iteration */
    float var_eps;                 /* added to the sigma; finite, > 0 */
    uint32_t flags;                /* 0 */
    uint32_t reserved[2];          /* 0 */
} trhip_denoise_var_params;        /* 48 bytes */
int trhip_denoise_var_default_params(trhip_denoise_var_params* out);
int trhip_denoise_var(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* variance, uint32_t width, uint32_t height, const trhip_denoise_var_params* params,
                      float* out_xyzw, float* out_variance, trhip_stats* stats);
int trhip_denoise_var_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_variance, uint32_t width, uint32_t height,
                             const trhip_denoise_var_params* params, void* d_out_xyzw, void* d_out_variance, trhip_stats* stats);

/* ---- edge-aware upscaling of a low-resolution film (since ABI 3001, added without a version change: nothing existing moved) ----
 * Joint bilateral upsampling (Kopf et al. 2007): the path frame is rendered through a sensor of lower resolution, the feature planes through
 * both sensors, and the full-size film is reconstructed from the low one with the normal and plane-distance edge tests of trhip_denoise
 * between a full-size pixel and its low-resolution neighbours.  Base-colour demodulation puts material edges back at full resolution; a miss
 * carries exactly zero radiance (path and Whitted frames have no environment term), so silhouettes are put back by coverage.  Specified operation by
 * operation in docs/design/17-upscale.md; bit-reproducible.
 *   lo_xyzw, lo_planes   lo_height * lo_width float4 and * 3 float4: what trhip_render_path (or trhip_denoise, trhip_temporal*) and
 *                        trhip_render_aov wrote for the low-resolution sensor
 *   hi_planes            height * width * 3 float4: what trhip_render_aov wrote for the full-size sensor, at any spp
 *   out_xyzw             height * width float4, a full-size film state: into film.set_xyzw / save, and into trhip_denoise with hi_planes.  Its .w
 *                        lane is plane 0's weight of hi_planes BIT FOR BIT: the filter_weight_sum of a native frame with the guides' sampler
 *   out_mask             height * width bytes or NULL: 0 nothing (no weight, or no usable low pixel: colour 0), 1 guided, 2 unguided (no surface
 *                        pixel: bilinear over the plain low colours), 3 orphan — a full-size surface pixel that no low-resolution tap agreed
 *                        with, a feature the low frame missed: filled like 2, flagged, the caller's to re-render
 * lo_from_hi = (ax, bx, ay, by): full-size ARRAY pixel x lies at low-resolution array coordinate x * ax + bx (integers at pixel centres), likewise
 * y.  For two sensors of one camera with the optical axis at raster position o (o = -m03 / m00 of raster_to_camera): ax = res_lo.x / res_hi.x,
 * bx = (crop_min_hi.x + 0.5 - o_hi.x) * ax + o_lo.x - 0.5 - crop_min_lo.x (docs/design/17-upscale.md).
 * Low pixel q: trhip_denoise's Prepare gives (s, n, p, c), c demodulated with TRHIP_UPSCALE_DEMODULATE and, with TRHIP_UPSCALE_COVERAGE, divided by
 * v = H / A; plain colour u = xyz_to_rgb(xyz / w), valid iff w > 0 and u finite.  Full-size pixel with A = plane 0's weight, H = plane 1's:
 * A > 0 false gives (0, 0, 0, A).  A surface pixel (H > 0, H >= min_coverage * A, finite n, p, a, v) sums the (2 radius)^2 low pixels around its
 * position, j outer and i inner, with w = (k * wn) * wp: k the tent 1 - d / radius per axis, wn = g((1 - n.n_q) / sigma_normal),
 * wp = g(|n.(p_q - p)| / sigma_plane), g Tukey's biweight; taps off the image or with s false are skipped; c' = sum / ws, times a, times v.  Any
 * other pixel, and a surface pixel with ws = 0 or c' not finite, takes the bilinear mean of u over the valid ones of its four low pixels.
 * out = (rgb_to_xyz(c') * A, A).
 * TRHIP_ERR_INVALID, in this order, the parameter block before any handle: params NULL; an entry of lo_from_hi not finite, ax or ay outside
 * [1/4, 1], |bx| or |by| >= 2^20; radius not 1 or 2; sigma_normal, sigma_plane or albedo_floor not finite and > 0; min_coverage outside [0, 1];
 * unknown flag bits; reserved != 0; then a null pointer (out_mask and stats excepted); a zero dimension; out_xyzw or out_mask overlapping an
 * input or each other.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (64 bytes per low pixel, 65 per full-size pixel) do not fit in free
 * HBM, or an image of more than 2^20 pixels on a side.  stats (may be NULL): ms_total, ms_film and launches_film over the call's kernels.  The
 * _device variant takes DEVICE pointers for the five images and allocates nothing beyond the context's scratch.  The default parameters need no
 * context and no GPU: radius 2, flags 0, sigma_normal 0.25 (the denoiser's), sigma_plane 0.4 — of the swept cells the one with the lowest error against the
 * native frame (profiles/r14/upscale.txt) —, albedo_floor 1/64, min_coverage 0.5; they leave lo_from_hi zero, which is refused: the map has to be given. */
#define TRHIP_UPSCALE_DEMODULATE 1u
#define TRHIP_UPSCALE_COVERAGE 2u
typedef struct {
    float lo_from_hi[4];           /* ax, bx, ay, by: low-res array coordinate of high-res array pixel x is x * ax + bx */
    uint32_t radius;               /* 1 or 2: guided footprint of (2 radius)^2 low-res taps */
    uint32_t flags;                /* TRHIP_UPSCALE_DEMODULATE | TRHIP_UPSCALE_COVERAGE, or 0 (the default) */
    float sigma_normal;            /* the denoiser's edge tests, between a full-size pixel and a low one */
    float sigma_plane;
    float albedo_floor;            /* the denoiser's; finite, > 0 */
    float min_coverage;            /* the denoiser's surface-pixel rule, [0, 1] */
    uint32_t reserved[2];          /* 0 */
} trhip_upscale_params;            /* 48 bytes */
int trhip_upscale_default_params(trhip_upscale_params* out);
int trhip_upscale(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes, uint32_t width, uint32_t height,
                  const trhip_upscale_params* params, float* out_xyzw, uint8_t* out_mask, trhip_stats* stats);
int trhip_upscale_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes, uint32_t width,
                         uint32_t height, const trhip_upscale_params* params, void* d_out_xyzw, void* d_out_mask, trhip_stats* stats);

/* ---- display pass: metered exposure, tone curve and 8-bit encode of a film (since ABI 3001, added without a version change: nothing existing moved) ----
 * The last stage of a preview: the Float32 film state is metered, exposed, tone-mapped and encoded to 8-bit RGBA on the device, 4 bytes per pixel
 * instead of 16 for the host to fetch.  Specified operation by operation in docs/design/18-display.md; no transcendental function is evaluated, and the
 * result is bit-reproducible from run to run (the metering histogram is integer).
 *   xyzw               height * width float4: a film state, what trhip_render_path, trhip_denoise, trhip_temporal*, trhip_upscale wrote
 *   scale              the film's scale (film.jl: the factor of save)
 *   out_rgba           height * width * 4 bytes: R, G, B, A per pixel, A = 255 where the pixel's weight is not 0 and 0 elsewhere; row r of the output is row
 *                      height - 1 - r of the film with TRHIP_DISPLAY_FLIP_ROWS (the order save writes), row r otherwise
 *   out_histogram256   256 uint32 or NULL: the metered counts (all zero without TRHIP_DISPLAY_AUTO_EXPOSURE)
 *   state              16 bytes the CALLER owns, carried from frame to frame; all zero = no state.  trhip_display takes it in HOST memory (in and out),
 *                      trhip_display_device in DEVICE memory.  NULL: no state is read, none is kept.  Written only with AUTO_EXPOSURE.
 * Metering (AUTO_EXPOSURE only): a pixel counts iff w > 0 and Y = ((y / w as y * (1 / w)) * scale) satisfies 2^-20 <= Y < +Inf; its bin is
 * min((bits(Y) >> 20) - 856, 255): 256 bins, eight per octave from 2^-20 to 2^12, the lower edge of bin b being the float with bits (b + 856) << 20.
 * Resolve: total = sum of the counts.  total == 0: E = state.valid ? state.exposure : exposure, state = {E, state.valid, 0, 0}.  Otherwise b = the smallest
 * bin with cum(b) * 1000 >= total * percentile_permille, need = ceil(total * permille / 1000), Lm = L(b) + (float(need - cum(b - 1)) / float(hist[b])) *
 * (L(b + 1) - L(b)), Et = clamp(key / Lm, min_exposure, max_exposure), E = state.exposure + (Et - state.exposure) * adapt_rate when a valid state is given
 * and adapt_rate < 1, else Et; state = {E, 1, total, b}.  Without AUTO_EXPOSURE E = exposure.
 * Encode: c = what trhip_film_to_rgb computes before its clamp (XYZ -> RGB, divided by w and floored at 0 where w != 0, times scale), times E, capped at
 * 2^40; per channel t = c (CLAMP), (c * (1 + c / white^2)) / (1 + c) (REINHARD, extended), (c * (2.51 c + 0.03)) / (c * (2.43 c + 0.59) + 0.14) (ACES,
 * Narkowicz's fit); t clamped to [0, 1], NaN to 0; the byte is rint(t * 255), ties to even (LINEAR), or the number of k in 1..255 with t >= T[k] (SRGB),
 * T the table trhip_display_srgb_table returns: T[k] the smallest Float32 not below the sRGB EOTF of (k - 0.5) / 255.  Every byte is defined whatever the
 * film holds.  With CLAMP, LINEAR, no AUTO_EXPOSURE, exposure 1 and FLIP_ROWS the RGB bytes are the ones save writes for every pixel free of NaN.
 * TRHIP_ERR_INVALID, in this order, the parameter block before any handle: params NULL; curve > 2; transfer > 1; unknown flag bits; exposure, key,
 * min_exposure or max_exposure not finite and > 0; min_exposure > max_exposure; percentile_permille outside 1..1000; adapt_rate outside (0, 1]; white outside
 * [2^-10, 2^20]; scale not finite; reserved != 0; then a null pointer (state, histogram and stats excepted); a zero dimension; width * height >= 2^31;
 * out_rgba overlapping the input.  TRHIP_ERR_UNSUPPORTED: more than 65535 blocks of 16 pixels on a side, or the host variant's device copies (20 bytes
 * per pixel) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film and launches_film over the call's kernels: 3 with AUTO_EXPOSURE (meter,
 * resolve, encode), 1 without; their parts in ms_sub / launches_sub: [0] meter, [1] resolve, [2] encode; the 1 KiB histogram is cleared by a memset,
 * which is not counted.  The _device variant takes DEVICE pointers and allocates
 * nothing beyond a 1 KiB histogram and a 16-byte state slot kept on the context.  The default parameters need no context and no GPU: REINHARD, SRGB, both
 * flags, exposure 1, key 0.18, the median (500), adapt_rate 1, exposures within [2^-8, 2^8], white 4 — conventional values, not swept. */
#define TRHIP_DISPLAY_AUTO_EXPOSURE 1u
#define TRHIP_DISPLAY_FLIP_ROWS 2u
#define TRHIP_DISPLAY_CURVE_CLAMP 0u
#define TRHIP_DISPLAY_CURVE_REINHARD 1u
#define TRHIP_DISPLAY_CURVE_ACES 2u
#define TRHIP_DISPLAY_TRANSFER_LINEAR 0u
#define TRHIP_DISPLAY_TRANSFER_SRGB 1u
typedef struct {
    uint32_t curve;                /* 0 CLAMP, 1 REINHARD (extended), 2 ACES (Narkowicz's rational fit) */
    uint32_t transfer;             /* 0 LINEAR, 1 SRGB */
    uint32_t flags;                /* TRHIP_DISPLAY_AUTO_EXPOSURE | TRHIP_DISPLAY_FLIP_ROWS */
    float exposure;                /* the exposure when AUTO is off; the fallback when nothing could be metered */
    float key;                     /* luminance the metered percentile is mapped to */
    uint32_t percentile_permille;  /* 1..1000 */
    float adapt_rate;              /* (0, 1]; 1 = no smoothing */
    float min_exposure, max_exposure;
    float white;                   /* REINHARD's white point, in exposed units */
    uint32_t reserved[2];          /* 0 */
} trhip_display_params;            /* 48 bytes */
typedef struct {
    float exposure;
    uint32_t valid, counted, key_bin;
} trhip_display_state;             /* 16 bytes; all zero = no state */
int trhip_display_default_params(trhip_display_params* out);
/* out256[0] = 0, out256[k] = T[k]; no context, no GPU */
int trhip_display_srgb_table(float* out256);
int trhip_display(trhip_ctx* ctx, const float* xyzw, uint32_t width, uint32_t height, float scale, const trhip_display_params* params, trhip_display_state* host_state_inout,
                  uint8_t* out_rgba, uint32_t* out_histogram256, trhip_stats* stats);
int trhip_display_device(trhip_ctx* ctx, const void* d_xyzw, uint32_t width, uint32_t height, float scale, const trhip_display_params* params, void* d_state, void* d_out_rgba,
                         void* d_histogram256, trhip_stats* stats);

/* ---- temporal upsampling of jittered low-resolution path frames (since ABI 3001, added without a version change: nothing existing moved) ----
 * trhip_upscale rebuilds every full-size frame from one low-resolution estimate; with a low camera that is shifted by a sub-pixel offset every frame and a history
 * held at FULL size, detail below the low grid accumulates instead.  One fused pass: the low film is upscaled onto the full-size planes as trhip_upscale
 * does it (flags off), and blended into the previous frame's history, fetched through the previous full-size camera as trhip_temporal fetches it, with a
 * weight kappa in [0, 1] that says how directly a low sample observed the pixel.  Specified operation by operation in docs/design/19-temporal-upsample.md; bit-reproducible.
 *   lo_xyzw, lo_planes   what trhip_render_path and trhip_render_aov wrote for the (jittered) low-resolution sensor
 *   hi_planes            what trhip_render_aov wrote for the full-size sensor (any spp)
 *   history              height * width * 3 float4 in trhip_temporal's layout, or NULL: word 0 = (c.rgb, Omega), Omega an accumulated WEIGHT, not a frame count;
 *                        word 1 = (n, 1.0 if surface else 0.0); word 2 = (p, 0).  The out_history of the previous call.
 *   out_xyzw             height * width float4: a film state; .w is plane 0's weight of hi_planes bit for bit
 *   out_history          this frame's history
 *   out_mask             height * width bytes or NULL: trhip_upscale's class (0 nothing, 1 guided, 2 unguided, 3 orphan) + 4 where history was found
 * lo_from_hi as in trhip_upscale_params, for THIS frame's jittered low sensor; prev_world_to_pixel: trhip_sensor_world_to_pixel of the previous FULL-SIZE sensor.
 * Per full-size pixel: steps H1-H5 of trhip_upscale with guide_sigma_normal, guide_sigma_plane, min_coverage, radius and no flags give its colour c and class m; every
 * accepted guided tap also gives e = ((gy * gx) * wn) * wp, gx = max(1 - d_x * confidence_sharpness, 0) with d_x the tap's distance in low pixels, and kmax is the largest
 * e.  kappa = max(kmax, confidence_floor) for a guided pixel, confidence_floor for an orphan, 0 for a surface pixel nothing was found for.  A pixel that is no surface
 * pixel gets trhip_upscale's value and a zero history.  A surface pixel gathers four history taps as trhip_temporal does (a tap needs Omega > 0) and blends
 * Omega' = min(Omega_h + kappa, max_history), c' = c_h + (kappa / Omega') * (c - c_h); without history, or when the blend is not finite, c' = c and Omega' = kappa.
 * With history NULL out_xyzw and out_mask are trhip_upscale's bit for bit.
 * TRHIP_ERR_INVALID, in this order, the parameter block before any handle: params NULL; trhip_upscale's checks of lo_from_hi, radius, guide_sigma_normal,
 * guide_sigma_plane, min_coverage; flags != 0; reserved != 0; trhip_temporal's checks of prev_world_to_pixel, max_history, sigma_normal, sigma_plane;
 * confidence_floor outside (0, 1]; confidence_sharpness outside [0, 4]; then a null pointer (history, out_mask and stats excepted); a zero dimension; out_history
 * overlapping an input; out_xyzw or out_mask overlapping an input, out_history or each other.  TRHIP_ERR_UNSUPPORTED as trhip_upscale (the host variant's copies are
 * 64 bytes per low pixel and 161 per full-size pixel).  stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes DEVICE pointers and
 * allocates nothing.  The default parameters need no context and no GPU: radius 1, max_history 8, confidence_sharpness 2, confidence_floor 1/16 — of the swept cells
 * the one with the lowest error against the upscaled session (profiles/r16/temporal_upsample.txt) —, the sigmas of trhip_temporal and trhip_upscale, min_coverage 0.5;
 * they leave lo_from_hi and prev_world_to_pixel zero. */
typedef struct {
    float lo_from_hi[4];           /* ax, bx, ay, by of this frame's (jittered) low sensor, as in trhip_upscale_params */
    float prev_world_to_pixel[12]; /* trhip_sensor_world_to_pixel of the previous frame's FULL-SIZE sensor */
    float max_history;             /* cap of the accumulated weight, >= 1 */
    float sigma_normal;            /* the history taps: strict thresholds as in trhip_temporal_params: 0.25, 0.1 */
    float sigma_plane;
    float min_coverage;            /* the surface-pixel rule of both sizes, [0, 1] */
    float guide_sigma_normal;      /* the low taps: Tukey widths as in trhip_upscale_params: 0.25, 0.4 */
    float guide_sigma_plane;
    float confidence_floor;        /* kappa_0 in (0, 1]: the least weight of a guided pixel, and an orphan's */
    float confidence_sharpness;    /* rho in [0, 4]: the confidence falls to 0 at 1 / rho low pixels from a low pixel centre; 0: geometry alone decides */
    uint32_t radius;               /* 1 or 2 */
    uint32_t flags;                /* 0 */
    uint32_t reserved[2];          /* 0 */
} trhip_temporal_upsample_params;  /* 112 bytes */
int trhip_temporal_upsample_default_params(trhip_temporal_upsample_params* out);
int trhip_temporal_upsample(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes, const float* history,
                            uint32_t width, uint32_t height, const trhip_temporal_upsample_params* params, float* out_xyzw, float* out_history, uint8_t* out_mask,
                            trhip_stats* stats);
int trhip_temporal_upsample_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes,
                                   const void* d_history, uint32_t width, uint32_t height, const trhip_temporal_upsample_params* params, void* d_out_xyzw, void* d_out_history,
                                   void* d_out_mask, trhip_stats* stats);

/* ---- moving geometry in a preview: the id plane and motion-aware reprojection (since ABI 3001, added without a version change: nothing existing moved) ----
 * trhip_temporal looks for a pixel's history where its surface point lies NOW; on a rigid body that moved between the frames the point was elsewhere, and the
 * taps found there fail the plane test.  Two entry points close the gap: a per-pixel id plane that says which primitive a pixel shows, and trhip_temporal with a
 * per-body matrix that carries the pixel's surface back to where its body was.  Specified operation by operation in docs/design/20-motion.md; bit-reproducible.
 *
 * trhip_render_aov_ids: trhip_render_aov with a third, optional output.  out_planes and out_samples are trhip_render_aov's BIT FOR BIT for the same arguments.
 * Any output may be NULL (all three: TRHIP_ERR_INVALID).  out_ids: (crop height) * (crop width) trhip_aov_id records in [y][x] order, like out_planes.  Film pixel
 * (x, y) looks at its OWN spp records, [s][y - sb.min.y][x - sb.min.x], s = 0 .. spp-1 — not at the neighbours that reach it through the filter —: n_hit is the number
 * of them with prim >= 0, and among those whose t is not NaN the one with the smallest t gives prim, material and t (ties: the lowest s).  Without one:
 * prim = material = -1, t = +Inf (n_hit = 0 unless every hitting record's t is NaN).  prim is trhip_hit.prim: the ordered-primitive slot, prim_order[prim] the
 * caller's index.  One more launch (stats.ms_film includes it when out_planes is drawn; launches_film counts it); 16 bytes per film pixel beside trhip_render_aov's buffers. */
typedef struct {
    int32_t prim;      /* ordered-primitive slot of the nearest of the pixel's own camera samples, -1: none hit */
    int32_t material;  /* its material id as trhip_aov_sample.material, -1: none */
    float t;           /* its ray parameter, +Inf: none hit */
    uint32_t n_hit;    /* how many of the pixel's spp camera samples hit anything */
} trhip_aov_id;        /* 16 bytes */
int trhip_render_aov_ids(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, float* out_planes,
                         trhip_aov_sample* out_samples, trhip_aov_id* out_ids, trhip_stats* stats);
int trhip_render_aov_ids_device(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                                void* d_out_planes, void* d_out_samples, void* d_out_ids, trhip_stats* stats);

/* trhip_temporal_motion: trhip_temporal — its images, layouts, overlap rules and stats — with
 *   ids            height * width trhip_aov_id of the CURRENT frame (only prim is read)
 *   body_of_prim   n_prims uint32, indexed by ids.prim: the rigid body of the primitive; a value >= n_bodies (by convention 0xFFFFFFFF) means static.  May be NULL.
 *   bodies         n_bodies * 12 floats: per body a row-major 3 x 4 matrix prev_from_cur that maps a point of the body in THIS frame's world to where that point was
 *                  in the PREVIOUS frame's world.  The caller promises a rigid motion; nothing about the matrix is checked.  May be NULL.
 * A pixel is static when ids.prim < 0 or >= n_prims, when body_of_prim or bodies is NULL, or when its body index is >= n_bodies: it gets trhip_temporal's arithmetic
 * on its n and p untouched, bit for bit (no multiplication by an identity).  Otherwise p' = A (p, 1), component i = ((A[i][0]*p.x + A[i][1]*p.y) + A[i][2]*p.z) + A[i][3],
 * and n' the same without the last column, not renormalised; p' or n' not finite: no history.  p' is projected through prev_world_to_pixel, and n', p' stand for n, p in both
 * tap tests.  Blend, cap, the non-finite fallback and out_xyzw as in trhip_temporal.  out_history stores the CURRENT n and p: the next frame's previous world.
 * For ANY bit content of ids and body_of_prim the kernel reads only inside the three arrays: every index is range-checked before it addresses anything.
 * Shadows and reflections that a moving body drags over other surfaces are not re-projected: they lag by the history length (docs/design/20-motion.md);
 * trhip_temporal_clip_motion, below, clips them.
 * TRHIP_ERR_INVALID, in this order: params NULL; trhip_temporal's checks of the fields it shares, in its order; flags != 0; reserved != 0 (the parameter block first,
 * before any handle); then a null pointer (history, body_of_prim, bodies and stats excepted); a zero dimension; n_prims > 0 with body_of_prim NULL; n_bodies > 0 with
 * bodies NULL; out_history overlapping any input or out_xyzw.  out_xyzw may be xyzw.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (176 bytes per pixel, 4 per
 * primitive, 48 per body) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes DEVICE pointers for all eight
 * arrays and allocates nothing.  trhip_temporal_motion_default_params needs no context and no GPU: trhip_temporal_default_params' values, n_prims = n_bodies = 0. */
typedef struct {
    float prev_world_to_pixel[12]; /* as in trhip_temporal_params, and the four below */
    float max_history;
    float sigma_normal;
    float sigma_plane;
    float min_coverage;
    uint32_t n_prims;              /* entries of body_of_prim */
    uint32_t n_bodies;             /* matrices in bodies */
    uint32_t flags;                /* 0 */
    uint32_t reserved;             /* 0 */
} trhip_temporal_motion_params;    /* 80 bytes */
int trhip_temporal_motion_default_params(trhip_temporal_motion_params* out);
int trhip_temporal_motion(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim,
                          const float* bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* params, float* out_xyzw, float* out_history,
                          trhip_stats* stats);
int trhip_temporal_motion_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, const void* d_ids, const void* d_body_of_prim,
                                 const void* d_bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* params, void* d_out_xyzw, void* d_out_history,
                                 trhip_stats* stats);

/* trhip_temporal_clip_motion: trhip_temporal_motion — its arguments in its order, its body carry, its memory-safety promise — with trhip_temporal_clip's variance clipping of
 * the reprojected history colour, and a history length that is cut when a clip fires (docs/design/21-clip-motion.md is the specification).
 *   The window statistics are trhip_temporal_clip's on the CURRENT frame's n, p, c (same visiting order, counting rule, lo and hi): no motion enters them.
 *   p' and n' of trhip_temporal_motion project and validate the four taps.
 *   After c_h = sc / sb: per channel c_h = (c_h < lo) ? lo : ((c_h > hi) ? hi : c_h); clipped = any of the six comparisons held; N_h = sN / sb;
 *   if (clipped && clip_max_history < N_h) N_h = clip_max_history; then N1 = N_h + 1, the cap, the blend and the non-finite fallback of trhip_temporal.
 *   out_history stores the CURRENT n and p.
 * ids may be NULL when n_prims == 0: every pixel is then static, and the pass serves a static scene for its history shortening alone.
 * Every pixel static and clip_max_history = +Inf: trhip_temporal_clip's output bit for bit.  clip_gamma = +Inf: trhip_temporal_motion's bit for bit, whatever
 * clip_max_history is.  A NaN c_h is never "clipped".  clip_max_history = 0: a clipped pixel restarts (blend weight 1, N' = 1).
 * TRHIP_ERR_INVALID, in this order: params NULL; trhip_temporal_motion's block checks on base, in its order; clip_gamma NaN or < 0; clip_radius not 1, 2 or 3;
 * clip_max_history NaN or < 0; reserved2 != 0 (the parameter block first, before any handle); then trhip_temporal_motion's pointer, size and overlap checks, with ids
 * NULL-able only when n_prims == 0.  out_xyzw may be xyzw: the window reads neighbours' film pixels, so the host variant gives the result a film of its own and the device
 * variant writes through a film held by the context and copies, as trhip_temporal_clip does.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (192 bytes per
 * pixel, 4 per primitive, 48 per body) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film, launches_film = 1.
 * trhip_temporal_clip_motion_default_params needs no context and no GPU: trhip_temporal_motion_default_params' base, clip_gamma 4, clip_radius 3 and the
 * clip_max_history chosen by the sweep of profiles/r18/clip_motion.txt. */
typedef struct {
    trhip_temporal_motion_params base;
    float clip_gamma;         /* >= 0; +Inf: no clipping */
    uint32_t clip_radius;     /* 1, 2 or 3 */
    float clip_max_history;   /* >= 0; +Inf: the history length is never cut */
    uint32_t reserved2;       /* 0 */
} trhip_temporal_clip_motion_params; /* 96 bytes */
int trhip_temporal_clip_motion_default_params(trhip_temporal_clip_motion_params* out);
int trhip_temporal_clip_motion(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim,
                               const float* bodies, uint32_t width, uint32_t height, const trhip_temporal_clip_motion_params* params, float* out_xyzw, float* out_history,
                               trhip_stats* stats);
int trhip_temporal_clip_motion_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, const void* d_ids, const void* d_body_of_prim,
                                      const void* d_bodies, uint32_t width, uint32_t height, const trhip_temporal_clip_motion_params* params, void* d_out_xyzw,
                                      void* d_out_history, trhip_stats* stats);

/* trhip_temporal_upsample_motion: trhip_temporal_upsample — its arguments in its order, its images, layouts and stats — for a scene whose rigid bodies moved between the
 * frames, with ids, body_of_prim, bodies of trhip_temporal_motion directly after history (docs/design/22-upsample-motion.md is the specification).
 *   ids            height * width trhip_aov_id of the FULL-SIZE frame (only prim is read); may be NULL when n_prims == 0: every pixel is then static
 *   body_of_prim   n_prims uint32 as in trhip_temporal_motion; may be NULL
 *   bodies         n_bodies * 12 floats, prev_from_cur per body as in trhip_temporal_motion; may be NULL
 * Step U of trhip_temporal_upsample (the upscale onto the full-size planes, the class m, the confidence kappa) is unchanged: the low frame and the full-size planes are this
 * frame's.  A pixel that is no surface pixel is trhip_temporal_upsample's, and its id is not looked at.  A surface pixel is static or moving by trhip_temporal_motion's rule
 * (each test before the next one's memory is touched); a static pixel keeps the bits of p and n, a moving one gets p' = A (p, 1) and n' = A n (no last column) by
 * trhip_temporal_motion's two three-line products, and a non-finite component of either means no history.  p' is projected through prev_world_to_pixel, and n', p' stand
 * for n, p in both tap tests; the Omega > 0 rule, the sums, the blend, the cap and the non-finite fallback are trhip_temporal_upsample's.  out_history stores the CURRENT
 * n and p; out_mask is m + 4 where history was found.
 * Every pixel static: trhip_temporal_upsample's three outputs bit for bit.  history NULL: trhip_upscale's film and mask bit for bit, whatever the bodies are.  Words 1 and 2
 * of out_history and out_xyzw's .w never depend on the bodies.  For ANY bit content of ids and body_of_prim the kernel reads only inside its arrays.
 * TRHIP_ERR_INVALID, in this order: params NULL; trhip_temporal_upsample's block checks on base, in its order; motion_flags != 0; reserved2 != 0 (the parameter block first,
 * before any handle); then trhip_temporal_upsample's pointer, size and overlap checks with ids, body_of_prim and bodies counted among the inputs; n_prims > 0 with
 * body_of_prim or ids NULL; n_bodies > 0 with bodies NULL.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (64 bytes per low pixel, 177 per full-size pixel, 4 per
 * primitive, 48 per body) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes DEVICE pointers for all ten arrays
 * and allocates nothing.  trhip_temporal_upsample_motion_default_params needs no context and no GPU: trhip_temporal_upsample_default_params' base, both counts 0. */
typedef struct {
    trhip_temporal_upsample_params base;
    uint32_t n_prims;       /* entries of body_of_prim */
    uint32_t n_bodies;      /* matrices in bodies */
    uint32_t motion_flags;  /* 0 */
    uint32_t reserved2;     /* 0 */
} trhip_temporal_upsample_motion_params; /* 128 bytes */
int trhip_temporal_upsample_motion_default_params(trhip_temporal_upsample_motion_params* out);
int trhip_temporal_upsample_motion(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes,
                                   const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim, const float* bodies, uint32_t width, uint32_t height,
                                   const trhip_temporal_upsample_motion_params* params, float* out_xyzw, float* out_history, uint8_t* out_mask, trhip_stats* stats);
int trhip_temporal_upsample_motion_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes,
                                          const void* d_history, const void* d_ids, const void* d_body_of_prim, const void* d_bodies, uint32_t width, uint32_t height,
                                          const trhip_temporal_upsample_motion_params* params, void* d_out_xyzw, void* d_out_history, void* d_out_mask,
                                          trhip_stats* stats);

/* trhip_temporal_split: trhip_temporal_motion — its arguments, its parameter block, its body carry, its memory-safety promise — for a preview that keeps the first-hit direct
 * light out of the history (docs/design/23-direct-split.md is the specification), with
 *   direct         height * width * 4 floats, directly after xyzw: the film of the frame's direct light (xyz, w; w is not read).  May be NULL.
 * Step 0: B' = (B.x - D.x, B.y - D.y, B.z - D.z, B.w) with D = direct[pixel]; direct NULL: B' = B, the same bits.  Everything after it is trhip_temporal_motion on B': the
 * surface test, the body carry, the four taps, the blend, the fallback; a pixel that is no surface pixel gets out_xyzw = B' and twelve zero history words.  The history
 * then holds the indirect remainder alone; trhip_film_add puts the direct film back after the filter.
 * direct NULL, or all +0: trhip_temporal_motion's outputs bit for bit; with no table and no matrices as well, trhip_temporal's.  direct is read at the pixel's own place only.
 * ids may be NULL when n_prims == 0, as in trhip_temporal_clip_motion: every pixel is then static, and a static scene needs no id plane.
 * TRHIP_ERR_INVALID: trhip_temporal_motion's refusals in its order (ids NULL-able only when n_prims == 0), then out_history overlapping direct, then out_xyzw overlapping
 * direct.  out_xyzw may be xyzw.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (192 bytes per pixel, 4 per primitive, 48 per body) do not fit in free HBM.
 * stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes DEVICE pointers for all nine arrays and allocates nothing. */
int trhip_temporal_split(trhip_ctx* ctx, const float* xyzw, const float* direct, const float* planes, const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim,
                         const float* bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* params, float* out_xyzw, float* out_history,
                         trhip_stats* stats);
int trhip_temporal_split_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_direct, const void* d_planes, const void* d_history, const void* d_ids,
                                const void* d_body_of_prim, const void* d_bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* params,
                                void* d_out_xyzw, void* d_out_history, trhip_stats* stats);

/* trhip_film_add: out.xyz = a.xyz + b.xyz, one Float32 addition per lane, and out.w = a.w, for two films of height * width * 4 floats.  out may be a.
 * TRHIP_ERR_INVALID, in this order: a null pointer (stats excepted); a zero dimension; out overlapping b.  TRHIP_ERR_UNSUPPORTED: the host variant's device copies (32 bytes
 * per pixel) do not fit in free HBM.  stats (may be NULL): ms_total, ms_film, launches_film = 1.  The _device variant takes DEVICE pointers and allocates nothing. */
int trhip_film_add(trhip_ctx* ctx, const float* a, const float* b, uint32_t width, uint32_t height, float* out, trhip_stats* stats);
int trhip_film_add_device(trhip_ctx* ctx, const void* d_a, const void* d_b, uint32_t width, uint32_t height, void* d_out, trhip_stats* stats);

/* SPPMIntegrator(camera, initial_search_radius, max_depth, n_iterations, photons_per_iteration)(scene)
 * (integrators/sppm.jl:108-173): per iteration a camera pass to the first diffuse vertex, a hash grid over the visible
 * points, a photon pass (Halton / radical_inverse, sampler/sampling.jl:43-60) and the Float64 pixel update; afterwards
 * _sppm_to_image + set_image! (film.jl:195-202).  out_xyzw: film_h * film_w * 4 (xyz, filter_weight_sum = 1).
 * photons_per_iteration <= 0: area(crop_bounds) like sppm.jl:121-124.  The film's crop must start at pixel (1, 1).
 * The camera pass of iteration k draws from the seeded stream (seed, pixel, sample k-1).  Photon contributions are added
 * with Float32 atomics as in the reference (sppm.jl:398-399): M, radius, N, Ld and the visible points are reproducible
 * bit for bit, τ (and the image) up to the summation order of ϕ.
 * A DirectionalLight has no sample_le in the reference (a photon that picks one ends the reference run at sppm.jl:361): the call
 * returns TRHIP_ERR_UNSUPPORTED, before any launch, when sample_discrete over the light power (sampling.jl:3-41) could pick one for
 * a photon of Halton indices 0 .. n_iterations * photons_per_iteration - 1 — its CDF interval has nonzero width (power (I·π)·r² > 0,
 * directional.jl:54-56; or every light's power is 0 and the uniform CDF gives it an interval), or it is the last light and some
 * index of the range has radical_inverse(0, index) == 1.0f (index ≡ 2^25 - 1 mod 2^25, the first at 2^25 - 1).  Otherwise the light
 * renders through the camera pass's direct term alone.
 * A GeometricPrimitive without a material (primitive.jl:1-9, material = nothing) is crossed as the reference crosses it
 * (sppm.jl:218-222, 380-410): the ray goes on from p + 1e-6 d along d at the same depth, with the same β and sampler dimensions;
 * a photon deposits at such a hit when its depth is > 1, as at any other hit.  Such a primitive still blocks shadow rays.  The
 * reference follows crossings without end; this call follows at most TRHIP_SPPM_MAX_CROSSINGS of them per camera path or photon,
 * and a call in which any path meets more returns TRHIP_ERR_UNSUPPORTED (the message names the cap and the number of paths over
 * it) and no image.  With such primitives in the scene max_depth may be at most 63 - TRHIP_SPPM_MAX_CROSSINGS. */
#define TRHIP_SPPM_MAX_CROSSINGS 8
int trhip_render_sppm(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, float initial_search_radius, int max_depth, uint32_t n_iterations,
                      int64_t photons_per_iteration, uint64_t seed, float* out_xyzw, trhip_stats* stats);
/* … with the reference's periodic image (integrators/sppm.jl:166-171: `iteration % write_frequency == 0 || iteration == n_iterations` -> _sppm_to_image,
 * set_image!, save): after every iteration k < n_iterations that write_frequency divides, `write` receives the image of the first k iterations (in out_xyzw, which the
 * call owns until it returns: film_h * film_w * 4) and returns 0 to go on; the last iteration's image is the call's result, as above.  The batches of iterations that
 * share traversal launches end at those iterations, so write_frequency = 1 (the reference's default) runs one iteration per batch — about 3x the time of a call without
 * a callback.  write == NULL or write_frequency == 0: trhip_render_sppm.  In a multi-GPU job every rank's callback runs (each holds the whole image after the iteration's
 * all-reduce; hosts let rank 0 write) and the return codes are max-reduced over the ranks before anyone acts on them: a failure on one rank ends the call on all. */
typedef int (*trhip_sppm_write_fn)(void* user, uint32_t iteration, const float* xyzw);
int trhip_render_sppm_ex(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, float initial_search_radius, int max_depth, uint32_t n_iterations,
                         int64_t photons_per_iteration, uint64_t seed, float* out_xyzw, trhip_stats* stats, uint32_t write_frequency, trhip_sppm_write_fn write, void* user);
/* SPPMPixel fields (sppm.jl:65-95) after the last trhip_render_sppm on this context, (film_h, film_w[, 3]) row-major; any
 * pointer may be NULL.  M, phi, vp_p, vp_beta: the last iteration's values before _update_pixels! cleared them.
 * info6 = grid resolution x y z, grid entries, photon hits inside the grid (all iterations), photons per iteration. */
int trhip_sppm_state(trhip_ctx* ctx, float* Ld3, float* tau3, float* radius, double* N, int64_t* M, float* phi3, float* vp_p3, float* vp_beta3, int64_t* info6);

/* save(film) minus the PNG encoder (film.jl:204-222): xyzw -> linear RGB in [0,1], H*W*3, rows not flipped. */
int trhip_film_to_rgb(trhip_ctx* ctx, const float* xyzw, uint32_t width, uint32_t height, float scale, float* out_rgb);

/* ---- kernel-level entry points (parity tests and micro-benchmarks) --------------------------------------------------
 * rays: n*8 floats (o.xyz, t_max, d.xyz, time) = Ray (ray.jl:1-6).
 * trhip_hit: t = ray.t_max after intersect!(bvh, ray) (accel/bvh.jl:212-258; +Inf on a miss), prim = ordered-primitive
 * slot of the hit (-1 on a miss), b1/b2 = first two barycentrics of a triangle hit (triangle_mesh.jl:217-218). */
typedef struct {
    float t;
    int32_t prim;
    float b1, b2;
} trhip_hit;
int trhip_trace_closest(trhip_ctx* ctx, const trhip_scene* scene, const float* rays, uint64_t n, trhip_hit* out);
/* intersect_p(bvh, ray)  accel/bvh.jl:260-299 */
int trhip_trace_any(trhip_ctx* ctx, const trhip_scene* scene, const float* rays, uint64_t n, uint8_t* occluded);
/* Same on device-resident buffers, `repeat` launches back to back; returns average kernel ms (HIP events) — used by bench.py. */
int trhip_trace_closest_device(trhip_ctx* ctx, const trhip_scene* scene, const void* d_rays, uint64_t n, void* d_hits, int repeat, double* avg_ms);
int trhip_trace_any_device(trhip_ctx* ctx, const trhip_scene* scene, const void* d_rays, uint64_t n, void* d_occluded, int repeat, double* avg_ms);

/* Visit counters of the last *_device trace call when "count_visits" is on: nodes, prims (closest) then nodes, prims (any-hit). */
int trhip_last_visit_counts(trhip_ctx* ctx, uint64_t* out4);
/* Of the last trace call of the kernel-level entry points — closest-hit OR any-hit: every one of them zeroes the counters first, an any-hit call leaves 0 handed back —
 * (trhip_trace_closest, trhip_trace_any, trhip_hit_geometry, *_device): rays traced, and how many of them the hybrid mode's certified walk handed to the
 * reference-order walk on the canonical tree (0 when the scene holds one tree).  The frame entry points report the same through trhip_stats.fallback_rays. */
int trhip_last_fallback_counts(trhip_ctx* ctx, uint64_t* out2);

/* Device time (ms, HIP events: upload of the primitive bounds to the last flatten kernel) of the last BVHAccel built by the device
 * SAH builder ("bvh_builder" = 3, accel/bvh.jl:55-206 replaced); 0 when the last commit used another builder. */
int trhip_last_bvh_build_ms(trhip_ctx* ctx, double* ms_device);

/* Geometry of a closest hit as the shading kernel rebuilds it (SurfaceInteraction, surface_interaction.jl:51-88,154-181;
 * BSDF frame materials/bsdf.jl:41-50): per ray 15 floats p(3) n(3) ns(3) wo(3) ss(3); zeros on a miss. */
int trhip_hit_geometry(trhip_ctx* ctx, const trhip_scene* scene, const float* rays, uint64_t n, float* out_geom15);

/* generate_ray(camera, sample) camera/perspective.jl:85-114 for n camera samples (film.xy, lens.xy, time) -> n*8 rays. */
int trhip_generate_rays(trhip_ctx* ctx, const trhip_sensor* sensor, const float* samples5, uint64_t n, float* out_rays8);

/* BSDF through a material (materials/material.jl + materials/bsdf.jl:79-193) for n shading frames frame9 = ng ns ss(=normalize(shading.∂p∂u)):
 *   mode 0: dirs6 = wo(3) wi(3)      -> out8 = f(3) pdf 0 0 0 0          (b(wo,wi,flags), compute_pdf)
 *   mode 1: dirs6 = wo(3) u(2) 0     -> out8 = wi(3) f(3) pdf type       (sample_f) */
int trhip_bsdf_query(trhip_ctx* ctx, const trhip_scene* scene, uint32_t material, int allow_multiple_lobes, int mode, int flags,
                     const float* frame9, const float* dirs6, uint64_t n, float* out8);

/* Film splat of caller-provided samples: add_sample! + merge_film_tile! in the reference's tile order
 * (film.jl:134-193, integrators/sampler.jl:24-52).  sample_L: n_sample_pixels*spp*3 as in trhip_last_sample_radiance;
 * p_film positions are regenerated from (seed, sample_offset). */
int trhip_film_accumulate(trhip_ctx* ctx, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, const float* sample_L,
                          float* out_xyzw);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -----------------------------------------------------
 * The scene is replicated; samples are independent.  A frame is sharded by global sample index (`sample_offset`: rank r of N
 * renders indices [r*spp_r, (r+1)*spp_r) of every pixel) into a private film; Film pixels are additive (xyz sums and
 * filter_weight_sum, film.jl:161-162, 190-191 — what merge_film_tile! relies on, film.jl:182-193), so ONE collective ends the frame.
 * The reference's only parallelism is Threads.@threads over tiles (integrators/sampler.jl:24) and photons (integrators/sppm.jl:334).
 *
 * trhip_comm_unique_id: rank 0 creates the 128-byte RCCL id (ncclGetUniqueId) and hands it to the other processes by any means
 *     (a file, MPI, torch.distributed's store ...).  trhip_comm_init: ncclCommInitRank on the context's GPU (collective: every
 *     rank calls it).  n_ranks == 1 is allowed (the collectives become copies).  RCCL is dlopen'ed on first use.
 * trhip_film_reduce: in-place ncclReduce(sum) of n_pixels x 4 floats (a device pointer, e.g. what trhip_render_path_device wrote)
 *     onto `root`; blocking.  trhip_film_allreduce: the same with every rank receiving the sum.
 * With a communicator, trhip_render_sppm shards the photon pass (rank r traces photon indices [r*P/N, (r+1)*P/N) of every
 *     iteration, sppm.jl:334) and all-reduces the per-pixel ϕ and M (sppm.jl:398-399) before _update_pixels! (sppm.jl:438-459):
 *     one exchange per iteration; every rank ends with the whole image.  The camera pass is replicated (1 path per pixel). */
#define TRHIP_UNIQUE_ID_BYTES 128
int trhip_comm_unique_id(uint8_t* out_id128);
int trhip_comm_init(trhip_ctx* ctx, const uint8_t* id128, int rank, int n_ranks);
int trhip_comm_destroy(trhip_ctx* ctx);
int trhip_comm_rank(const trhip_ctx* ctx, int* rank, int* n_ranks); /* 0 / 1 without a communicator */
int trhip_film_reduce(trhip_ctx* ctx, void* d_xyzw, uint64_t n_pixels, int root);
int trhip_film_allreduce(trhip_ctx* ctx, void* d_xyzw, uint64_t n_pixels);

/* ---- options ------------------------------------------------------------------------------------------------------- */
/* "count_visits" (0/1): instrumented traversal kernels fill nodes_visited / prims_tested.
 * "batch_paths": paths in flight per wavefront batch (0 = size from free HBM, the default).
 * "timing" (0/1): per-kernel HIP-event timing in trhip_stats (default 1).
 * "traversal" (1/2/3/4/6): 1 = literal accel/bvh.jl loop, 2 = children-in-parent nodes with per-lane ray replacement,
 *     3 (default) = 2 with the leaves of a wave postponed and tested together, 4 = 8-wide nodes with quantised child boxes walked
 *     in the binary tree's depth-first order (th_trace8.h; measured on par with 3); scenes 4 cannot take (foreign
 *     trees whose boxes do not nest, leaves of several primitives, more than 8 spheres, spheres not committed as a chain — see
 *     "compose_spheres") and rays it cannot take (a zero direction component) run 3; 6 = 3 with two rays per lane (th_trace4.h: better
 *     lane use, no fewer instructions: measured slower).  Same results bit for bit.
 * "compose_spheres" (-1/0/1): how trhip_scene_commit places up to 8 spheres of a scene that also has triangles: 1 = as a chain of
 *     single-sphere leaves above the triangles' subtree (what traversal 4 needs), 0 = inside one SAH tree, -1 (default) = 1 when
 *     "traversal" is 4 at commit time.  Either tree is a valid BVHAccel: results differ only in exact-t ties.
 * "overlap" (0/1): shadow rays of depth d on a second stream beside the closest-hit pass of depth d+1 (default 0: no gain any more).
 *     "stream2_priority" (-1/0/1): that stream's priority: lowest (default: the closest-hit rays are the critical path), the
 *     default level, highest; read when the streams are created (first render of a context).
 * "pipelines" (1..8): wavefront batches in flight at once (default 1).
 * "film_fused" (0/1, default 1): the path integrator's ray generation writes every sample's radiance record in the film pass's own layout, with its splat
 *     descriptor, so that a frame needs no memset of the records and no pack / re-lay pass before the gather (film.jl:134-164 replaced; same film bit for bit).
 * "film_relayout" (0/1, default 1): records that were not written that way (film_fused 0, Whitted, trhip_film_accumulate, …) are copied into that layout on their
 *     way to the gather, when there is room for the copy; 0 = their descriptors are written in place and the gather reads the sample-major records.  Same film
 *     bit for bit.  Both options concern filter radii in (0, 1] alone: any other radius takes the one wide film pass (film positions, 1 x 4 blocks per thread).
 * "bvh_builder" (-1/0/1/2/3): how trhip_scene_commit builds the BVH: 0 = binned SAH on the host, 1 = linear BVH on the device
 *     (Morton keys, radix sort, Karras hierarchy; 25-35 % more node visits per ray), 3 = the host builder's binned SAH run on the
 *     device (the same tree, 18 ms per million primitives instead of ~170 ms; scenes it cannot take go to the host builder),
 *     2 = the reference's own construction node for node (see trhip_scene_commit), -1 (default) = 3 from 64 Ki primitives on,
 *     0 below.  Every one of these trees is a valid BVHAccel: results differ only in exact-t ties.
 * "slab_margin_log2" (0..20, default 14): traversal 2 / 3 add to the reference's box test (bounds.jl:180-200) the two slab
 *     clauses it lost — it keeps the larger of the x and y exits — evaluated on boxes grown by 2^-N x the ray's reach; boxes on
 *     the path to a sphere keep the reference's test alone.  Fewer boxes visited, same results bit for bit;
 *     0 = the reference's test alone (its exact visit set, and the traversal tail that comes with it).
 * "tiny_scene_prims" (0..255): scenes of at most this many primitives are committed as ONE leaf (default 16; 0 = never).
 *     Read by trhip_scene_commit; results do not depend on it except through the order coincident hits are visited in.
 * "streaming" (-1/0/1): PathIntegrator on scenes with a real BVH as a streaming wavefront: rays that exceed a fetch budget
 *     are suspended and resumed in the next round instead of holding up their launch; same result bit for bit.  0 (default):
 *     never — since "slab_margin_log2" removed the 10^5-fetch rays it only costs; 1 always; -1 automatic (frames of
 *     at most 96 camera samples per primitive).  "stream_budget_min" (default 2048), "stream_budget_shift" (12) and
 *     "stream_list_cap" (0 = automatic) tune it.
 * "occluder_pretest" (0/1, default 1): any-hit rays test the scene's (at most 16) largest triangles first and go through the
 *     hierarchy only when none of them stops the ray; exact (th_trace2.h, k_any_occluders).
 * "sppm_batch": SPPM iterations whose camera / photon paths share the traversal launches (default 0 = as many as fit in
 *     free HBM, at most 128); the result does not depend on it.
 * "denoise_lds" (bit mask 0..3, default 3): bit i set = iteration i of trhip_denoise (i = 0, 1: steps 1, 2) stages its blocks' pixels and halo in LDS
 *     instead of gathering them from memory (measured 7 % and 3 % faster); same result bit for bit (th_denoise.h).
 * "temporal_patch" (0/1, default 1): which lane of trhip_temporal's kernel computes which pixel — 0 film order (a wave is 64 pixels of a row), 1 the à-trous
 *     kernel's patches of 16 x 4 pixels per wave (measured 11 % faster); same result bit for bit (th_temporal.h).  No effect on
 *     trhip_temporal_clip, whose kernel has the patch mapping only.
 * "denoise_var_lds" (bit mask 0..3, default 3): as "denoise_lds", for trhip_denoise_var's iterations (measured 17 % and 16 % faster staged; th_denoise_var.h).
 * "leaf_kernel" (0/1): one-leaf scenes (tiny_scene_prims) run the dedicated uniform-walk kernel instead of traversal 2 (default 1).
 * "band_tile_rows": PathIntegrator frames whose per-sample buffers (24 B per camera sample) do not fit in HBM are rendered in bands of
 *     whole 16-row tile rows into the same film — bit-identical to one band (tiles reach a film pixel in the reference's order either
 *     way); this option forces bands of N tile rows (tests; 0 = automatic).  trhip_last_sample_radiance needs a one-band frame.
 * "debug_trace_budget": DIAGNOSTIC ONLY, traversal abandons rays after this many node fetches (results wrong). */
int trhip_set_option(trhip_ctx* ctx, const char* name, int64_t value);
/* Whether this BUILD of the library carries the kernel families behind `name = value` (traversal 4 / 6 / 7, leaf_queue, leaf_sorted,
 * bvh_builder 1 exist only in the EXPERIMENTS build, -DTRHIP_EXPERIMENTS): 1 yes, 0 no (trhip_set_option would return
 * TRHIP_ERR_UNSUPPORTED).  A property of the binary: needs no context and no GPU — test suites decide at COLLECTION which variants exist. */
int trhip_option_in_build(const char* name, int64_t value);

/* The deterministic elementary functions of trace_detmath.h for hosts that cannot include a C header
 * (fn: 0 sin, 1 cos, 2 tan, 3 atan2(y, x), 4 acos, 5 log, 6 / 7 the sin / cos part of tm_sincosf); y may be NULL unless
 * fn == 3.  Needs no GPU. */
int trhip_detmath_f32(int fn, const float* x, const float* y, uint64_t n, float* out);
/* The same functions as the GPU kernels evaluate them (one thread per element): host and device must agree bit for bit. */
int trhip_detmath_f32_device(trhip_ctx* ctx, int fn, const float* x, const float* y, uint64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* TRACEHIP_H */
