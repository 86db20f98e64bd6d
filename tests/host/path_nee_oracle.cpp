// tests/host/path_nee_oracle.cpp — TEST INFRASTRUCTURE ONLY: the model of the walk of a path-env frame with next-event estimation (docs/design/28-path-nee.md), from the oracle
// alone.  It includes the oracle's API unit unchanged, as tests/host/path_env_oracle.cpp does (tests/path_nee_model.py builds it with oracle/Makefile's compiler and flags), and
// takes the scene handles liboracle.so made.  The one function it adds restates path_li (oracle/orc_render.h) line for line with the escape record, its suppressed mark, and —
// after the point-light term of every vertex and before the `depth == max_depth` break — the geometry of the vertex's next-event estimate: the technique, the direction, the
// BSDF's density and f |cos|, the throughput and the shadow ray's verdict.  A map-chosen direction depends on (u0, u1) alone, so the caller (numpy, tests/sky_is_model.py)
// computes env_sample for every (sample, vertex) up front and hands the directions in; it finishes the estimate with env_pdf and env_eval and sums in depth order.
#include "../../oracle/orc_api.cpp"

namespace {
constexpr int VF = 16;  // floats per (sample, vertex): see path_nee_walk
enum : int { V_NONE = 0, V_SPECULAR = 1, V_MAP = 2, V_BSDF = 3 };                       // [0] the vertex and its technique
enum : int { R_NO_DIRECTION = 0, R_BLACK = 1, R_OPEN = 2, R_OCCLUDED = 3 };            // [1] what became of the estimate
struct Escape {
    int depth = 0;
    RGB beta{0.0f};
    V3 dir{0.0f};
    bool suppressed = false;
};
RGB path_li_nee(Scene& scene, Ray ray, const SeededSampler& smp, int max_depth, float mix, const float* env_dirs, Escape& esc, float* vtx) {
    const uint8_t NS = BSDF_ALL & ~BSDF_SPECULAR;
    RGB L(0.0f), beta(1.0f);
    int depth = 1;
    bool prev_non_specular = false;
    while (depth <= max_depth) {
        SurfaceInteraction si;
        if (!scene_intersect(scene, ray, si)) {
            esc.depth = depth;
            esc.beta = beta;
            esc.dir = ray.d;
            esc.suppressed = prev_non_specular;
            break;
        }
        const BSDF bsdf = compute_scattering(scene, si, true);
        if (!bsdf.valid) {
            ray = spawn_ray_dir(si, ray.d);
            continue;
        }
        const V3 wo = -ray.d;
        const uint32_t v = (uint32_t)(depth - 1);
        float* V = vtx + (size_t)v * VF;
        const uint64_t shadow0 = counters().shadow;
        const RGB dl = beta * uniform_sample_one_light(scene, si, bsdf, smp.u(ts_vertex_dim(v, TS_V_LIGHT_PICK)));
        L = L + dl;
        V[9] = beta.x, V[10] = beta.y, V[11] = beta.z;
        V[12] = dl.x, V[13] = dl.y, V[14] = dl.z;
        V[15] = (float)(counters().shadow - shadow0);
        // ---- the next-event estimate of the map: steps 1 - 9 of the definition, up to what needs the map ----
        if (bsdf.num_components(NS) == 0) {
            V[0] = (float)V_SPECULAR;
            prev_non_specular = false;
        } else {
            prev_non_specular = true;
            bool have = true;
            V3 wi(0.0f);
            if (smp.u(ts_vertex_dim(v, TS_V_LIGHT_PICK)) < mix) {
                V[0] = (float)V_MAP;
                wi = V3(env_dirs[3 * v], env_dirs[3 * v + 1], env_dirs[3 * v + 2]);
            } else {
                V[0] = (float)V_BSDF;
                const BSDFSample s = bsdf_sample_f(bsdf, wo, V2{smp.u(ts_vertex_dim(v, TS_V_SCATTER_U0)), smp.u(ts_vertex_dim(v, TS_V_SCATTER_U1))}, NS);
                if (s.pdf == 0.0f)
                    have = false;
                else
                    wi = s.wi;
            }
            if (!have) {
                V[1] = (float)R_NO_DIRECTION;
            } else {
                const float pb = bsdf.pdf(wo, wi, NS);
                const RGB fa = bsdf.f(wo, wi, NS) * std::fabs(dot(wi, si.sh_n));
                V[2] = wi.x, V[3] = wi.y, V[4] = wi.z;
                V[5] = pb;
                V[6] = fa.x, V[7] = fa.y, V[8] = fa.z;
                if (is_black(fa)) {
                    V[1] = (float)R_BLACK;
                } else {  // (the caller discards the verdict where the mixture density turns out not to be positive: no ray there)
                    Ray r = spawn_ray_dir(si, wi);
                    V[1] = (float)(scene_intersect_p(scene, r) ? R_OCCLUDED : R_OPEN);
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
    return L;
}
}  // namespace

extern "C" {

int path_nee_vertex_floats() { return VF; }

// env_dirs: spp * n_sample_pixels * max_depth * 3, env_sample of every (sample, vertex)'s (TS_V_LIGHT_U0, TS_V_LIGHT_U1).
// out_L: spp * n_sample_pixels * 3: the point-light radiance alone, raw (trhip_render_path's).  out_rec: * 8 = beta.xyz, depth (0 = none), dir.xyz, 1 where suppressed.
// out_vtx: * max_depth * 16, zero where the path has no such vertex: [0] V_*, [1] R_*, [2..4] wi, [5] the BSDF's density, [6..8] f |cos|, [9..11] beta,
// [12..14] the point-light addend beta * uniform_sample_one_light, [15] the shadow rays it cast.  All indexed as orc_render's out_sample_L.
int path_nee_walk(void* sp, const orc_sensor* sn, int64_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, float mix, const float* env_dirs, float* out_L, float* out_rec,
                  float* out_vtx) {
    OrcScene* s = (OrcScene*)sp;
    if (!s->committed) return -1;
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
                Escape esc;
                const RGB l = path_li_nee(s->scene, ray, smp, max_depth, mix, env_dirs + at * max_depth * 3, esc, out_vtx + at * max_depth * VF);
                out_L[3 * at] = l.x, out_L[3 * at + 1] = l.y, out_L[3 * at + 2] = l.z;
                const float r[8] = {esc.beta.x, esc.beta.y, esc.beta.z, (float)esc.depth, esc.dir.x, esc.dir.y, esc.dir.z, esc.suppressed ? 1.0f : 0.0f};
                std::memcpy(out_rec + 8 * at, r, sizeof r);
                smp.start_next_sample();
            }
        }
    return 0;
}

}  // extern "C"
