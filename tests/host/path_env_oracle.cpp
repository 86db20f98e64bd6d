// tests/host/path_env_oracle.cpp — TEST INFRASTRUCTURE ONLY: the model of a path-env frame's walk (docs/design/26-path-env.md), from the oracle alone.  It includes the oracle's
// API unit unchanged, so it is compiled against the very headers liboracle.so is made of (tests/path_env_model.py builds it with oracle/Makefile's compiler and flags) and
// takes the scene handles that library made.  The one function it adds restates path_li (oracle/orc_render.h) line for line with ONE change — where scene_intersect fails
// the path records its escape (depth, beta, the ray's direction) before it ends — and returns, per camera sample, the RAW radiance L (no NaN rule) and that record.
// tests/test_path_env_api.py pins the restated loop to orc_render's per-sample path radiance bit for bit.
#include "../../oracle/orc_api.cpp"

namespace {
struct Escape {
    int depth = 0;
    RGB beta{0.0f};
    V3 dir{0.0f};
};
// path_li with the escape record; every other line is orc_render.h's
RGB path_li_escape(Scene& scene, Ray ray, const SeededSampler& smp, int max_depth, Escape& esc) {
    RGB L(0.0f), beta(1.0f);
    int depth = 1;
    while (depth <= max_depth) {
        SurfaceInteraction si;
        if (!scene_intersect(scene, ray, si)) {
            esc.depth = depth;
            esc.beta = beta;
            esc.dir = ray.d;
            break;
        }
        const BSDF bsdf = compute_scattering(scene, si, true);
        if (!bsdf.valid) {
            ray = spawn_ray_dir(si, ray.d);
            continue;
        }
        const V3 wo = -ray.d;
        const uint32_t v = (uint32_t)(depth - 1);
        L = L + beta * uniform_sample_one_light(scene, si, bsdf, smp.u(ts_vertex_dim(v, TS_V_LIGHT_PICK)));
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

// out_L: spp * n_sample_pixels * 3, raw.  out_rec: spp * n_sample_pixels * 8 = beta.xyz, depth (0 = none), dir.xyz, 0.  out_cam: optional, spp * n_sample_pixels * 8: the
// camera ray (o.xyz, t_max, d.xyz, time) and out_film: optional, * 2: camera_sample.film.  All indexed as orc_render's out_sample_L.
int path_env_walk(void* sp, const orc_sensor* sn, int64_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, float* out_L, float* out_rec, float* out_cam, float* out_film) {
    OrcScene* s = (OrcScene*)sp;
    if (!s->committed) return -1;
    const Film film = make_film(sn);
    const PerspectiveCamera cam = make_camera(sn);
    const Bounds2 sb = get_sample_bounds(film);
    const int sbw = (int)(sb.p_max.x - sb.p_min.x) + 1, sbh = (int)(sb.p_max.y - sb.p_min.y) + 1;
    const size_t n_pix = (size_t)sbw * sbh;
    SeededSampler smp(spp, seed, sample_offset);
    for (float py = sb.p_min.y; py <= sb.p_max.y; py += 1.0f)
        for (float px = sb.p_min.x; px <= sb.p_max.x; px += 1.0f) {
            const V2 pixel{px, py};
            smp.start_pixel(pixel);
            while (smp.has_next_sample()) {
                const CameraSample cs = smp.get_camera_sample(pixel);
                const Ray ray = generate_ray(cam, cs);
                Escape esc;
                const RGB l = path_li_escape(s->scene, ray, smp, max_depth, esc);
                const size_t pix = (size_t)(py - sb.p_min.y) * sbw + (size_t)(px - sb.p_min.x);
                const size_t at = (size_t)(smp.current_sample - 1) * n_pix + pix;
                out_L[3 * at] = l.x, out_L[3 * at + 1] = l.y, out_L[3 * at + 2] = l.z;
                const float r[8] = {esc.beta.x, esc.beta.y, esc.beta.z, (float)esc.depth, esc.dir.x, esc.dir.y, esc.dir.z, 0.0f};
                std::memcpy(out_rec + 8 * at, r, sizeof r);
                if (out_cam) {
                    const float c[8] = {ray.o.x, ray.o.y, ray.o.z, ray.t_max, ray.d.x, ray.d.y, ray.d.z, ray.time};
                    std::memcpy(out_cam + 8 * at, c, sizeof c);
                }
                if (out_film) out_film[2 * at] = cs.film.x, out_film[2 * at + 1] = cs.film.y;
                smp.start_next_sample();
            }
        }
    return 0;
}

// The film of per-sample radiances `L3` (indexed as above; the caller has applied the NaN rule): orc_render.h's render() with the integrator's value read from the array —
// its tiles in k order, its pixels and samples in its order, add_sample and merge_film_tile.  out_xyzw: height * width * 4.
int path_env_film(const orc_sensor* sn, int64_t spp, uint64_t seed, uint32_t sample_offset, const float* L3, float* out_xyzw) {
    Film film = make_film(sn);
    const Bounds2 sb = get_sample_bounds(film);
    const V2 extent{sb.p_max.x - sb.p_min.x, sb.p_max.y - sb.p_min.y};
    const int tile_size = 16;
    const long long width = (long long)std::floor((extent.x + tile_size) / tile_size), height = (long long)std::floor((extent.y + tile_size) / tile_size);
    const long long total_tiles = width * height - 1;
    const int sbw = (int)(sb.p_max.x - sb.p_min.x) + 1, sbh = (int)(sb.p_max.y - sb.p_min.y) + 1;
    const size_t n_pix = (size_t)sbw * sbh;
    for (long long k = 0; k <= total_tiles; ++k) {
        const float tx = (float)(k % width), ty = (float)(k / width);
        SeededSampler smp(spp, seed, sample_offset);
        const V2 tb_min{sb.p_min.x + tx * tile_size, sb.p_min.y + ty * tile_size};
        const V2 tb_max{jl_min(tb_min.x + (tile_size - 1), sb.p_max.x), jl_min(tb_min.y + (tile_size - 1), sb.p_max.y)};
        FilmTile tile(film, Bounds2{tb_min, tb_max});
        for (float py = tb_min.y; py <= tb_max.y; py += 1.0f)
            for (float px = tb_min.x; px <= tb_max.x; px += 1.0f) {
                const V2 pixel{px, py};
                smp.start_pixel(pixel);
                while (smp.has_next_sample()) {
                    const CameraSample cs = smp.get_camera_sample(pixel);
                    const size_t pix = (size_t)(py - sb.p_min.y) * sbw + (size_t)(px - sb.p_min.x);
                    const float* l = L3 + ((size_t)(smp.current_sample - 1) * n_pix + pix) * 3;
                    add_sample(tile, cs.film, RGB(l[0], l[1], l[2]), 1.0f);
                    smp.start_next_sample();
                }
            }
        merge_film_tile(film, tile);
    }
    for (size_t i = 0; i < film.pixels.size(); ++i) {
        const Pixel& p = film.pixels[i];
        const float o[4] = {p.xyz.x, p.xyz.y, p.xyz.z, p.filter_weight_sum};
        std::memcpy(out_xyzw + 4 * i, o, sizeof o);
    }
    return 0;
}

}  // extern "C"
