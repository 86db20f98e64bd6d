// tests/host/path_emit_oracle.cpp — TEST INFRASTRUCTURE ONLY: the model of an emit frame (docs/design/29-path-emit.md), from the oracle alone.  It includes the oracle's API
// unit unchanged, as tests/host/path_nee_oracle.cpp does (tests/path_emit_model.py builds it with oracle/Makefile's compiler and flags), and takes the scene handles
// liboracle.so made.  path_emit_walk restates path_li (oracle/orc_render.h) line for line with the emitted term at every hit and — after the point-light term of every
// vertex and before the `depth == max_depth` break — the vertex's next-event estimate towards the emitter set: pick, point, the densities, f |cos|, the contribution and
// the shadow ray's verdict within its reach.  The table (the 64-byte records, the cdf, the per-material Le) comes from the caller: numpy builds it
// (tests/path_emit_model.py) from path_emit_prims' vertices; the caller also sums in depth order.  path_emit_sample is the sampler's arithmetic on its own, which the tests
// pin to the numpy one.
#include "../../oracle/orc_api.cpp"

namespace {
constexpr int VF = 16;  // floats per (sample, vertex): see path_emit_walk
enum : int { V_NONE = 0, V_SPECULAR = 1, V_NEE = 2, V_HITS_ONLY = 3 };                   // [0] the vertex
enum : int { R_NO_RAY = 0, R_BLACK = 1, R_OPEN = 2, R_OCCLUDED = 3 };                    // [1] what became of the estimate
enum : int { E_NONE = 0, E_COUNTED = 1, E_SUPPRESSED = 2 };                             // [15] the emitted term
constexpr uint32_t HITS_ONLY = 1u;

struct Table {
    const float* tri;  // 16 n: {p0, P} {p1, A} {p2, slot} {Le, 0}
    const float* cdf;  // n + 1
    uint32_t n;
    const float* mat_le;  // 4 per material
    int n_mat;
};

uint32_t pick(const float* T, uint32_t n, float u) {  // the largest k in [0, n - 1] with T[k] <= u, by a fixed number of steps
    uint32_t lo = 0u;
    for (uint32_t step = n > 1u ? 1u << (31 - __builtin_clz(n - 1u)) : 0u; step; step >>= 1) {
        const uint32_t k = lo + step;
        if (k <= n - 1u && T[k] <= u) lo = k;
    }
    return lo;
}
V3 point(V3 p0, V3 p1, V3 p2, float u0, float u1) {
    const float s = std::sqrt(u0);
    const float b0 = 1.0f - s;
    const float b1 = u1 * s;
    const float b2 = (1.0f - b0) - b1;
    return (b0 * p0 + b1 * p1) + b2 * p2;
}

void path_li_emit(Scene& scene, Ray ray, const SeededSampler& smp, int max_depth, const Table& tb, float scale, uint32_t flags, float* vtx) {
    const uint8_t NS = BSDF_ALL & ~BSDF_SPECULAR;
    RGB beta(1.0f);
    int depth = 1;
    bool prev_specular = false;
    while (depth <= max_depth) {
        SurfaceInteraction si;
        if (!scene_intersect(scene, ray, si)) break;
        const uint32_t v = (uint32_t)(depth - 1);
        float* V = vtx + (size_t)v * VF;
        // 1. the emitted term
        if (si.prim && si.prim->kind == Primitive::TRIANGLE && si.prim->material >= 0 && si.prim->material < tb.n_mat) {
            const float* le = tb.mat_le + 4 * si.prim->material;
            if (le[0] != 0.0f || le[1] != 0.0f || le[2] != 0.0f) {
                if (depth == 1 || prev_specular || (flags & HITS_ONLY)) {
                    const float ex = le[0] * scale, ey = le[1] * scale, ez = le[2] * scale;
                    V[12] = beta.x * ex, V[13] = beta.y * ey, V[14] = beta.z * ez;
                    V[15] = (float)E_COUNTED;
                } else {
                    V[15] = (float)E_SUPPRESSED;
                }
            }
        }
        const BSDF bsdf = compute_scattering(scene, si, true);
        if (!bsdf.valid) {
            ray = spawn_ray_dir(si, ray.d);
            continue;
        }
        const V3 wo = -ray.d;
        const uint64_t shadow0 = counters().shadow;
        const RGB dl = beta * uniform_sample_one_light(scene, si, bsdf, smp.u(ts_vertex_dim(v, TS_V_LIGHT_PICK)));
        V[5] = beta.x, V[6] = beta.y, V[7] = beta.z;
        V[8] = dl.x, V[9] = dl.y, V[10] = dl.z;
        V[11] = (float)(counters().shadow - shadow0);
        // 3. next-event estimation towards the emitters
        if (bsdf.num_components(NS) == 0) {
            V[0] = (float)V_SPECULAR;
            prev_specular = true;
        } else if (flags & HITS_ONLY) {
            V[0] = (float)V_HITS_ONLY;
            prev_specular = false;
        } else {
            V[0] = (float)V_NEE;
            prev_specular = false;
            V[1] = (float)R_NO_RAY;
            const uint32_t dim = (uint32_t)TS_DIM_EMIT_BASE + 3u * v;
            const float xi = smp.u(dim), u0 = smp.u(dim + 1u), u1 = smp.u(dim + 2u);
            const uint32_t j = pick(tb.cdf, tb.n, xi);
            const float* r = tb.tri + 16 * (size_t)j;
            const V3 p0(r[0], r[1], r[2]), p1(r[4], r[5], r[6]), p2(r[8], r[9], r[10]);
            const V3 y = point(p0, p1, p2, u0, u1);
            const V3 w = y - si.p;
            const float d2 = dot(w, w);
            if (d2 != 0.0f) {
                const float dist = std::sqrt(d2);
                const V3 wi = w / dist;
                const V3 nx = cross(p1 - p0, p2 - p0);
                const float nl = norm(nx);
                const V3 n_l = nx / nl;
                const float cl = std::fabs(dot(n_l, wi));
                const float pa = r[3] / r[7];
                const float pn = pa * d2;
                const float pl = pn / cl;
                if (pl > 0.0f && pl != INF32) {
                    const RGB fa = bsdf.f(wo, wi, NS) * std::fabs(dot(wi, si.sh_n));
                    if (is_black(fa)) {
                        V[1] = (float)R_BLACK;
                    } else {
                        const float lx = r[12] * scale, ly = r[13] * scale, lz = r[14] * scale;
                        const float tx = fa.x * lx, ty = fa.y * ly, tz = fa.z * lz;
                        const float dx = tx / pl, dy = ty / pl, dz = tz / pl;
                        V[2] = beta.x * dx, V[3] = beta.y * dy, V[4] = beta.z * dz;
                        Ray sr = spawn_ray_dir(si, wi);
                        sr.t_max = dist * 0.999f;
                        const uint64_t keep = counters().shadow;
                        V[1] = (float)(scene_intersect_p(scene, sr) ? R_OCCLUDED : R_OPEN);
                        counters().shadow = keep;  // (the emitter rays are counted from the verdicts)
                    }
                }
            }
        }
        if (depth == max_depth) break;
        const V2 u{smp.u(ts_vertex_dim(v, TS_V_BSDF_U0)), smp.u(ts_vertex_dim(v, TS_V_BSDF_U1))};
        const BSDFSample s = bsdf_sample_f(bsdf, wo, u, BSDF_ALL);
        if (s.pdf == 0.0f || is_black(s.f)) break;
        beta = beta * (s.f * std::fabs(dot(s.wi, si.sh_n)) / s.pdf);
        const float by = to_Y(beta);
        if (by < 0.25f) {
            const float cont = jl_min(1.0f, by);
            if (smp.u(ts_vertex_dim(v, TS_V_RR)) > cont) break;
            beta = beta / cont;
        }
        ray = spawn_ray_dir(si, s.wi);
        depth += 1;
    }
}
}  // namespace

extern "C" {

int path_emit_vertex_floats() { return VF; }

// Per ordered primitive slot of the committed tree: the world-space vertices (zeros for a sphere), the material (-1: none) and the kind (0 triangle, 1 sphere, 2 other).
int path_emit_prims(void* sp, float* out_v9, int32_t* out_material, int32_t* out_kind) {
    OrcScene* s = (OrcScene*)sp;
    if (!s->committed) return -1;
    const std::vector<Primitive>& ps = s->scene.aggregate.primitives;
    for (size_t k = 0; k < ps.size(); ++k) {
        float* o = out_v9 + 9 * k;
        std::memset(o, 0, 9 * sizeof(float));
        out_material[k] = ps[k].material;
        out_kind[k] = ps[k].kind == Primitive::TRIANGLE ? 0 : ps[k].kind == Primitive::SPHERE ? 1 : 2;
        if (ps[k].kind == Primitive::TRIANGLE) {
            V3 vs[3];
            tri_vertices(ps[k].triangle, vs);
            for (int j = 0; j < 3; ++j) o[3 * j] = vs[j].x, o[3 * j + 1] = vs[j].y, o[3 * j + 2] = vs[j].z;
        }
    }
    return 0;
}

// pick and point for `count` triples (xi, u0, u1): the emitter, the point and P_j / A_j
void path_emit_sample(const float* tri, const float* cdf, uint32_t n, const float* u3, int64_t count, uint32_t* out_index, float* out_point3, float* out_pdf) {
    for (int64_t i = 0; i < count; ++i) {
        const uint32_t j = pick(cdf, n, u3[3 * i]);
        const float* r = tri + 16 * (size_t)j;
        const V3 y = point(V3(r[0], r[1], r[2]), V3(r[4], r[5], r[6]), V3(r[8], r[9], r[10]), u3[3 * i + 1], u3[3 * i + 2]);
        out_index[i] = j;
        out_point3[3 * i] = y.x, out_point3[3 * i + 1] = y.y, out_point3[3 * i + 2] = y.z;
        out_pdf[i] = r[3] / r[7];
    }
}

// out_vtx: spp * n_sample_pixels * max_depth * 16, zero where the path has no such vertex: [0] V_*, [1] R_*, [2..4] c, [5..7] beta, [8..10] the point-light addend
// beta * uniform_sample_one_light, [11] the shadow rays it cast, [12..14] the emitted addend beta * (Le * scale), [15] E_*.  Indexed as orc_render's out_sample_L.
int path_emit_walk(void* sp, const orc_sensor* sn, int64_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const float* tri, const float* cdf, uint32_t n, const float* mat_le,
                   int n_mat, float scale, uint32_t flags, float* out_vtx) {
    OrcScene* s = (OrcScene*)sp;
    if (!s->committed) return -1;
    const Table tb{tri, cdf, n, mat_le, n_mat};
    const Film film = make_film(sn);
    const PerspectiveCamera cam = make_camera(sn);
    const Bounds2 sb = get_sample_bounds(film);
    const int sbw = (int)(sb.p_max.x - sb.p_min.x) + 1, sbh = (int)(sb.p_max.y - sb.p_min.y) + 1;
    const size_t n_pix = (size_t)sbw * sbh;
    std::memset(out_vtx, 0, (size_t)spp * n_pix * max_depth * VF * sizeof(float));
    SeededSampler smp(spp, seed, sample_offset);
    for (float py = sb.p_min.y; py <= sb.p_max.y; py += 1.0f)
        for (float px = sb.p_min.x; px <= sb.p_max.x; px += 1.0f) {
            const V2 pixel{px, py};
            smp.start_pixel(pixel);
            while (smp.has_next_sample()) {
                const CameraSample cs = smp.get_camera_sample(pixel);
                const Ray ray = generate_ray(cam, cs);
                const size_t pix = (size_t)(py - sb.p_min.y) * sbw + (size_t)(px - sb.p_min.x);
                const size_t at = (size_t)(smp.current_sample - 1) * n_pix + pix;
                path_li_emit(s->scene, ray, smp, max_depth, tb, scale, flags, out_vtx + at * max_depth * VF);
                smp.start_next_sample();
            }
        }
    return 0;
}

}  // extern "C"
