// rt_render: headless driver of the C++ host layer (include/raytracer.hpp) --
// what the reference's binary does per frame, minus the window: pick a scene
// from the table, set it up (load OBJ, build BSP/HLBVH, upload), feed camera
// keys and commands, render progressive iterations, and write the frame.
//
//   rt_render --list-scenes
//   rt_render --scene NAME [--res WxH] [--spp N | --samples N] [--keys K1,K2 --updates N]
//             [--selection K] [--selection2 K] [--use-texture K] [--uv-scale A,B]
//             [--subdiv K] [--camera-constant C] [--device-build]
//             [--env-rgba FILE --env-size WxH] [--tex-rgba FILE --tex-size WxH]
//             [--models DIR] [--out PREFIX]
//             [--noise-target T [--noise-batch B] [--noise-allow F]]
//                                        (a path-mode scene: render B (16) iterations at a time
//                                        until at most F (0) x pixels have a relative standard
//                                        error above T, or --samples / --spp (1024) iterations
//                                        are done; the JSON line gains "noise": {iterations,
//                                        pixels, above, nonfinite, max_rel_err}, and --out
//                                        writes PREFIX.noise.f32, the H*W map; an untiled
//                                        render only: refused with --comm-file / --nranks)
//             [--adaptive-target T [--adaptive-min N] [--adaptive-vote pixel|tile] [--noise-batch B]]
//                                        (a path-mode scene: adaptive sampling, render_adaptive --
//                                        B (16) iterations at a time for the pixels (or 8x8 tiles,
//                                        the default vote) that have fewer than N (16) samples or a
//                                        relative standard error above T, until none is left or
//                                        --samples / --spp (1024) iterations are done; the JSON
//                                        line gains "adaptive": {iterations, pixels, live_next,
//                                        above, nonfinite, total_samples, min_count, max_count,
//                                        max_rel_err}, and --out writes PREFIX.count.u32, the H*W
//                                        sample counts; refused with --comm-file / --nranks and
//                                        with --noise-target)
//             [--denoise [--denoise-levels L] [--denoise-sigma-l S] [--denoise-sigma-z Z]]
//                                        (a path-mode scene with at least 2 iterations: the frame
//                                        through the variance-guided a-trous filter, rt_denoise --
//                                        L (5) levels, luminance and depth tolerances S (4) and Z (1);
//                                        enables the noise estimate if no other flag did; --out
//                                        also writes PREFIX.denoised.f32 (H*W*4 float32) and
//                                        PREFIX.denoised.rgba8 (its sRGB frame); refused with
//                                        --comm-file / --nranks)
//             [--temporal-frames N [--temporal-history M] [--temporal-normal-min D] [--temporal-plane-tol P]]
//                                        (a path-mode scene: after the --updates, N frames of --spp (1)
//                                        iterations each with the --keys held -- temporal_step: every
//                                        frame is blended with the history reprojected from the camera
//                                        before it, rt_temporal_accumulate, at most M (32) frames long,
//                                        rejecting taps whose normal differs (dot below D, 0.9) or that
//                                        lie off the pixel's plane (P (0.01) x depth); --out writes
//                                        PREFIX.temporal.f32 (the integrated frame, H*W*4 float32),
//                                        PREFIX.temporal.len.u32 (H*W history lengths),
//                                        PREFIX.temporal.denoised.f32 and PREFIX.temporal.denoised.rgba8
//                                        (through rt_temporal_variance and rt_denoise_filter, with the
//                                        parameters of --denoise --denoise-levels / --denoise-sigma-l /
//                                        --denoise-sigma-z if given: no progressive frame is rendered, so
//                                        PREFIX.denoised.* is not written) beside the progressive frame's
//                                        files; refused with --comm-file / --nranks, --noise-target,
//                                        --adaptive-target and --samples)
//             [--guide-objects]          (with --denoise or --temporal-frames: their guide also holds
//                                        the analytic objects of the scene's mode -- the two balls of
//                                        W8E1..W8E3, the holdout plane of W9E2 / W9E3 --, which the
//                                        primary ids do not name: set_guide_objects,
//                                        rt_denoise_guide_objects; a mode without them is not changed;
//                                        refused without one of the two flags)
//   rt_render ... --nranks N --rank R --comm-file PATH [--comm-token T] [--device D]
//                                        (one process per GPU: rank R renders its
//                                        interleaved tiles, rank 0 gathers the frame
//                                        over RCCL and writes it; rank 0 publishes the
//                                        communicator id in PATH, tagged with T -- any
//                                        string unique to the launch, e.g. a job id, the
//                                        same on every rank; default $RT_COMM_TOKEN --
//                                        and the other ranks take only a file with
//                                        their T, never a previous launch's; without a
//                                        token PATH must be fresh; device defaults to R)
//   rt_render --camera-test K1,K2 N      (CPU: eye after N controller updates)
//   rt_render --jitter SUBDIV HEIGHT     (CPU: the jitter table)
//
// --out writes PREFIX.accum.f32 (H*W*4 float32), PREFIX.ids.u32 (H*W) and
// PREFIX.rgba8 (the sRGB frame); one JSON summary line goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "raytracer.hpp"

using namespace raytracer;

static std::vector<std::string> split(const std::string& s, char c)
{
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, c))
        if (!t.empty()) out.push_back(t);
    return out;
}

static std::string jstr(const std::string& s)
{
    std::string o = "\"";
    for (char ch : s) {
        if (ch == '"' || ch == '\\') o += '\\';
        o += ch;
    }
    return o + "\"";
}

static std::string hexf(float f)
{
    char b[32];
    std::snprintf(b, sizeof b, "%a", (double)f);
    return jstr(b);
}

static const char* mode_name(std::optional<rt_mode> m)
{
    rt_mode_desc d;
    return m && rt_mode_describe(*m, &d) == RT_OK ? d.name : nullptr;
}

static std::string cam_json(const Camera& c)
{
    auto v = [](const Vec3& a) { return "[" + hexf(a[0]) + "," + hexf(a[1]) + "," + hexf(a[2]) + "]"; };
    return "{\"eye\":" + v(c.eye) + ",\"target\":" + v(c.target) + ",\"up\":" + v(c.up) +
           ",\"constant\":" + hexf(c.constant) + "}";
}

static void write_file(const std::string& path, const void* p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char*>(p), (std::streamsize)n);
    if (!f) throw Error(RT_E_INVALID, "cannot write " + path);
}

// the communicator id through a file: rank 0 writes "RTCOMMID <token>\n" and the
// id (to PATH.tmp, then renames, so a reader never sees a partial file), the
// other ranks wait for a file that carries their own token.  A file left by an
// earlier launch (another token) is never taken: its id has no rank 0 any more,
// and ncclCommInitRank would wait for it forever.
static void publish_comm_id(const std::string& path, const std::string& token, uint8_t id[RT_COMM_ID_BYTES],
                            uint32_t rank)
{
    if (token.find('\n') != std::string::npos) throw Error(RT_E_INVALID, "--comm-token: no newlines");
    const std::string head = "RTCOMMID " + token + "\n";
    if (rank == 0) {
        std::remove(path.c_str());   // a stale file goes before the new id exists
        if (int r = rt_comm_unique_id(id)) throw Error(r, rt_last_error(nullptr));
        std::string buf = head;
        buf.append(reinterpret_cast<const char*>(id), RT_COMM_ID_BYTES);
        write_file(path + ".tmp", buf.data(), buf.size());
        if (std::rename((path + ".tmp").c_str(), path.c_str()) != 0) throw Error(RT_E_INVALID, "cannot publish " + path);
        return;
    }
    for (int i = 0; i < 1200; i++) {   // up to 2 minutes
        std::ifstream f(path, std::ios::binary);
        std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (buf.size() == head.size() + RT_COMM_ID_BYTES && buf.compare(0, head.size(), head) == 0) {
            std::memcpy(id, buf.data() + head.size(), RT_COMM_ID_BYTES);
            return;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    throw Error(RT_E_NOT_READY, "no communicator id for token '" + token + "' in " + path);
}

static std::string default_models_dir(const char* argv0)
{
    // <repo>/02562_raytracer_amd/bin/rt_render -> <repo>/assets/models
    std::string p(argv0);
    const size_t k = p.rfind('/');
    std::string dir = k == std::string::npos ? "." : p.substr(0, k);
    return dir + "/../../assets/models";
}

// the command line: bare flags and `--name value` pairs; numbers as atoi / atof read them (garbage is 0)
struct Args {
    std::vector<std::string> words;
    bool has(const std::string& name) const   // the flag is there
    {
        for (const auto& s : words)
            if (s == name) return true;
        return false;
    }
    const std::string* str(const std::string& name) const   // the word after `name`, null without one
    {
        for (size_t i = 0; i + 1 < words.size(); i++)
            if (words[i] == name) return &words[i + 1];
        return nullptr;
    }
    template <class T>
    T num(const std::string& name, T otherwise) const
    {
        const std::string* s = str(name);
        if (!s) return otherwise;
        if constexpr (std::is_floating_point_v<T>) return (T)std::atof(s->c_str());
        else return (T)std::atoi(s->c_str());
    }
    std::optional<std::pair<uint32_t, uint32_t>> size(const std::string& name) const   // `name WxH`
    {
        const std::string* s = str(name);
        if (!s) return std::nullopt;
        unsigned w = 0, h = 0;
        if (std::sscanf(s->c_str(), "%ux%u", &w, &h) != 2) throw Error(RT_E_INVALID, name + " WxH");
        return std::make_pair((uint32_t)w, (uint32_t)h);
    }
};

// `file_option FILE` with `size_option WxH`: the file's raw RGBA8 texels to set(texels, width, height)
template <class Set>
static void read_rgba(const Args& args, const std::string& file_option, const std::string& size_option, Set set)
{
    const std::string* path = args.str(file_option);
    if (!path) return;
    const auto size = args.size(size_option);
    if (!size) throw Error(RT_E_INVALID, file_option + " needs " + size_option + " WxH");
    std::vector<uint8_t> texels((size_t)size->first * size->second * 4);
    std::ifstream f(*path, std::ios::binary);
    f.read(reinterpret_cast<char*>(texels.data()), (std::streamsize)texels.size());
    if (!f) throw Error(RT_E_INVALID, "cannot read " + *path);
    set(texels.data(), size->first, size->second);
}

// What is for an untiled state: the noise estimate and the counts are H x W maps, the filters need
// every pixel's neighbours, and --comm-file tiles the render for any rank count (--nranks 1 too),
// which packs the buffers per tile.  A row: the option, whether it is a bare flag, and who the
// refusal names for it.  The estimates' rows are checked before the options' consistency, the
// filters' rows after it.
static const struct {
    const char* option;
    bool flag;
    const char* who;
} kUntiled[] = {{"--noise-target", false, "--noise-target does"},
                {"--adaptive-target", false, "--adaptive-target / --adaptive-min / --adaptive-vote do"},
                {"--adaptive-min", false, "--adaptive-target / --adaptive-min / --adaptive-vote do"},
                {"--adaptive-vote", false, "--adaptive-target / --adaptive-min / --adaptive-vote do"},
                {"--denoise", true, "--denoise does"},
                {"--temporal-frames", false, "--temporal-frames does"}};
enum { kUntiledEstimates = 0, kUntiledFilters = 4, kUntiledEnd = 6 };

static void refuse_tiled(const Args& args, int from, int to)
{
    if (args.num<uint32_t>("--nranks", 1) <= 1 && !args.str("--comm-file")) return;
    for (int i = from; i < to; i++)
        if (kUntiled[i].flag ? args.has(kUntiled[i].option) : args.str(kUntiled[i].option) != nullptr)
            throw Error(RT_E_UNSUPPORTED, std::string(kUntiled[i].who) + " not go with --comm-file / --nranks (a tiled render)");
}

int main(int argc, char** argv)
{
    try {
        const Args args{std::vector<std::string>(argv + 1, argv + argc)};
        if (args.has("--list-scenes")) {
            for (const auto& s : get_scenes()) {
                const char* m = mode_name(s.mode());
                const char* rm = mode_name(s.render_mode());
                const char* am = mode_name(s.analytic_mode());
                const char* wm = mode_name(s.worksheet1_mode());
                const char* km = mode_name(s.kernel_mode());
                std::printf("{\"name\":%s,\"shader\":%s,\"mode\":%s,\"render_mode\":%s,\"analytic_mode\":%s,"
                            "\"worksheet1_mode\":%s,\"kernel_mode\":%s,\"model\":%s,\"res\":[%u,%u],"
                            "\"vertex_type\":%s,"
                            "\"traverse_type\":%s,\"background_hdri\":%s,\"camera\":%s}\n",
                            jstr(s.name).c_str(), jstr(s.shader).c_str(), m ? jstr(m).c_str() : "null",
                            rm ? jstr(rm).c_str() : "null", am ? jstr(am).c_str() : "null",
                            wm ? jstr(wm).c_str() : "null", km ? jstr(km).c_str() : "null",
                            s.model ? jstr(*s.model).c_str() : "null", s.res.first, s.res.second,
                            s.vertex_type == VertexType::Combined ? "\"Combined\"" : "\"Split\"",
                            s.traverse_type == TraverseType::Bsp ? "\"BSP\"" : "\"BVH\"",
                            s.background_hdri ? jstr(*s.background_hdri).c_str() : "null",
                            cam_json(s.camera).c_str());
            }
            return 0;
        }
        if (const std::string* k = args.str("--camera-test")) {
            CameraController ctl;
            for (const auto& name : split(*k, ',')) ctl.handle_camera_commands(key_from_name(name), true);
            Camera c;
            const int n = std::atoi(argc > 3 ? argv[3] : "1");
            for (int i = 0; i < n; i++) ctl.update_camera(c);
            std::printf("%s\n", cam_json(c).c_str());
            return 0;
        }
        if (args.str("--jitter")) {
            const double h = argc > 3 ? std::atof(argv[3]) : 512.0;
            for (const auto& j : compute_jitters(1.0 / h, args.num<uint32_t>("--jitter", 0)))
                std::printf("%s %s\n", hexf(j[0]).c_str(), hexf(j[1]).c_str());
            return 0;
        }
        const std::string* name = args.str("--scene");
        if (!name) {
            std::fprintf(stderr, "usage: rt_render --list-scenes | --scene NAME [options] (see the source header)\n");
            return 2;
        }
        RenderOptions opt;
        opt.models_dir = args.str("--models") ? *args.str("--models") : default_models_dir(argv[0]);
        opt.resolution = args.size("--res");
        opt.device_build = args.has("--device-build");
        const uint32_t nranks = args.num<uint32_t>("--nranks", 1), rank = args.num<uint32_t>("--rank", 0);
        if (nranks == 0 || rank >= nranks) throw Error(RT_E_INVALID, "--rank must be below --nranks");
        if (nranks > 1 && !args.str("--comm-file")) throw Error(RT_E_INVALID, "--nranks needs --comm-file PATH");
        const bool noise = args.str("--noise-target"), adaptive = args.str("--adaptive-target");
        refuse_tiled(args, kUntiledEstimates, kUntiledFilters);
        if (!adaptive && (args.str("--adaptive-min") || args.str("--adaptive-vote")))
            throw Error(RT_E_INVALID, "--adaptive-min / --adaptive-vote need --adaptive-target T");
        if (adaptive && noise) throw Error(RT_E_INVALID, "--adaptive-target does not go with --noise-target");
        // the denoise filter needs a noise state: a path mode
        const bool denoise = args.has("--denoise"), temporal = args.str("--temporal-frames");
        if (!denoise && (args.str("--denoise-levels") || args.str("--denoise-sigma-l") || args.str("--denoise-sigma-z")))
            throw Error(RT_E_INVALID, "--denoise-levels / --denoise-sigma-l / --denoise-sigma-z need --denoise");
        refuse_tiled(args, kUntiledFilters, kUntiledEnd);
        const auto path_scene = [&] {
            const auto row = mode_of_shader(find_scene(*name).shader);
            return row && row->family == RT_FAMILY_PATH;
        };
        const uint32_t dn_levels = args.num<uint32_t>("--denoise-levels", 5);
        const float dn_sigma_l = args.num<float>("--denoise-sigma-l", 4.0f), dn_sigma_z = args.num<float>("--denoise-sigma-z", 1.0f);
        if (denoise) {
            if (dn_levels < 1 || dn_levels > 5 || !(dn_sigma_l > 0.0f) || !(dn_sigma_z > 0.0f))
                throw Error(RT_E_INVALID, "--denoise-levels in 1..5, --denoise-sigma-l and --denoise-sigma-z > 0");
            if (!path_scene()) throw Error(RT_E_UNSUPPORTED, "--denoise: the scene's mode keeps no noise state (a path mode only)");
        }
        // temporal accumulation reprojects between whole frames of a path mode, one camera move per frame
        if (!temporal && (args.str("--temporal-history") || args.str("--temporal-normal-min") || args.str("--temporal-plane-tol")))
            throw Error(RT_E_INVALID, "--temporal-history / --temporal-normal-min / --temporal-plane-tol need --temporal-frames N");
        if (temporal && (noise || adaptive || args.str("--samples")))
            throw Error(RT_E_INVALID, "--temporal-frames does not go with --noise-target, --adaptive-target or --samples");
        const int tp_frames = args.num<int>("--temporal-frames", 0), tp_history = args.num<int>("--temporal-history", 32);
        const float tp_normal_min = args.num<float>("--temporal-normal-min", 0.9f);
        const float tp_plane_tol = args.num<float>("--temporal-plane-tol", 0.01f);
        if (temporal) {
            if (tp_frames < 1 || tp_history < 1 || !(tp_plane_tol >= 0.0f) || tp_normal_min != tp_normal_min)
                throw Error(RT_E_INVALID, "--temporal-frames and --temporal-history >= 1, --temporal-plane-tol >= 0");
            if (args.num<int>("--spp", 1) < 1) throw Error(RT_E_INVALID, "--temporal-frames: --spp >= 1");
            if (!path_scene())
                throw Error(RT_E_UNSUPPORTED, "--temporal-frames: the scene's mode writes no per-iteration records (a path mode only)");
        }
        // the guide with objects is the filters' guide: there is none to change without one of them
        const bool guide_objects = args.has("--guide-objects");
        if (guide_objects && !denoise && !temporal)
            throw Error(RT_E_INVALID, "--guide-objects needs --denoise or --temporal-frames N (it changes their guide)");
        int vote = RT_ADAPT_TILE;
        if (const std::string* v = args.str("--adaptive-vote")) {
            if (*v == "pixel") vote = RT_ADAPT_PIXEL;
            else if (*v != "tile") throw Error(RT_E_INVALID, "--adaptive-vote pixel|tile");
        }
        GpuHandles gpu(args.num<int>("--device", (int)rank));
        RenderState rs(gpu, find_scene(*name), opt);
        if (const std::string* cf = args.str("--comm-file")) {
            uint8_t id[RT_COMM_ID_BYTES];
            const char* et = std::getenv("RT_COMM_TOKEN");
            const std::string token = args.str("--comm-token") ? *args.str("--comm-token") : (et ? et : "");
            publish_comm_id(*cf, token, id, rank);
            rs.set_tiling(nranks, rank, id);
        }
        read_rgba(args, "--env-rgba", "--env-size", [&](const uint8_t* p, uint32_t w, uint32_t h) { rs.set_environment_map(p, w, h); });
        read_rgba(args, "--tex-rgba", "--tex-size", [&](const uint8_t* p, uint32_t w, uint32_t h) { rs.set_texture_image(p, w, h); });
        if (args.str("--selection")) rs.set_selection1(args.num<uint32_t>("--selection", 0));
        if (args.str("--selection2")) rs.set_other_material(args.num<uint32_t>("--selection2", 0));
        if (args.str("--use-texture") || args.str("--uv-scale")) {
            float a = 1.0f, b = 1.0f;
            if (const std::string* s = args.str("--uv-scale"))
                if (std::sscanf(s->c_str(), "%f,%f", &a, &b) != 2) throw Error(RT_E_INVALID, "--uv-scale A,B");
            rs.set_texture(args.num<uint32_t>("--use-texture", 0), {a, b});
        }
        if (args.str("--subdiv")) rs.set_subdivision_level(args.num<uint32_t>("--subdiv", 0));
        if (args.str("--camera-constant")) rs.update_camera_constant(args.num<float>("--camera-constant", 0.0f));
        if (const std::string* k = args.str("--keys")) {
            for (const auto& kn : split(*k, ',')) rs.input_alt(key_from_name(kn), true);
            const int n = args.num<int>("--updates", 1);
            for (int i = 0; i < n; i++) rs.update();
        } else {
            rs.update();
        }
        // --denoise: the noise estimate from iteration 0 on, unless --noise-target / --adaptive-target enable it
        // (with --temporal-frames it only carries the filter's parameters: no progressive frame is rendered)
        if (denoise && !temporal && !noise && !adaptive) rs.enable_noise();
        if (guide_objects) rs.set_guide_objects(true);   // (before enable_temporal below)
        uint32_t frames = 0;
        std::string noise_json;
        const std::string* const out = args.str("--out");
        // --noise-target and --adaptive-target: at most `cap` iterations, `batch` at a time
        const uint32_t cap = args.num<uint32_t>("--samples", args.num<uint32_t>("--spp", 1024)), spp = args.num<uint32_t>("--spp", 1);
        const uint32_t batch = args.num<uint32_t>("--noise-batch", 16);
        if (noise) {   // render until converged (render_until)
            rt_noise_summary ns;
            const uint32_t its = rs.render_until(args.num<float>("--noise-target", 0.0f), cap, batch,
                                                 args.num<double>("--noise-allow", 0.0), 1e-3f, &ns);
            frames = (its + batch - 1) / batch;
            if (out && its >= 2) {
                const auto nm = rs.noise_map();
                write_file(*out + ".noise.f32", nm.data(), nm.size() * 4);
            }
            char b[256];
            std::snprintf(b, sizeof b,
                          ",\"noise\":{\"iterations\":%u,\"pixels\":%llu,\"above\":%llu,\"nonfinite\":%llu,"
                          "\"max_rel_err\":%s}",
                          its, (unsigned long long)ns.pixels, (unsigned long long)ns.above,
                          (unsigned long long)ns.nonfinite, hexf(ns.max_rel_err).c_str());
            noise_json = b;
        } else if (adaptive) {   // adaptive sampling (render_adaptive)
            rs.enable_adaptive(args.num<float>("--adaptive-target", 0.0f), 1e-3f, args.num<uint32_t>("--adaptive-min", 16), vote);
            rt_adaptive_summary as;
            const uint32_t its = rs.render_adaptive(cap, batch, &as);
            frames = (its + batch - 1) / batch;
            if (out) {
                const auto cn = rs.sample_counts();
                write_file(*out + ".count.u32", cn.data(), cn.size() * 4);
            }
            char b[384];
            std::snprintf(b, sizeof b,
                          ",\"adaptive\":{\"iterations\":%u,\"pixels\":%llu,\"live_next\":%llu,\"above\":%llu,"
                          "\"nonfinite\":%llu,\"total_samples\":%llu,\"min_count\":%u,\"max_count\":%u,\"max_rel_err\":%s}",
                          its, (unsigned long long)as.pixels, (unsigned long long)as.live_next,
                          (unsigned long long)as.above, (unsigned long long)as.nonfinite,
                          (unsigned long long)as.total_samples, as.min_count, as.max_count, hexf(as.max_rel_err).c_str());
            noise_json = b;
        } else if (temporal) {   // N frames with the keys held (temporal_step); the progressive frame stays as it is
            rs.enable_temporal((uint32_t)tp_history, tp_normal_min, tp_plane_tol);
            for (int i = 0; i < tp_frames; i++) rs.temporal_step(spp);
            frames = (uint32_t)tp_frames;
        } else if (args.str("--samples")) {   // the progressive loop, SetSamples
            rs.set_samples(args.num<uint32_t>("--samples", 0), true);
            while (rs.step()) frames++;
        } else {
            rs.render(spp);
            frames = 1;
        }
        const rt_ray_counts c = rs.last_counts();
        if (rank != 0) return 0;   // the frame is rank 0's
        if (out) {
            const auto f = rs.frame();
            const auto ids = rs.hit_ids();
            const auto rgba = rs.frame_rgba8();
            write_file(*out + ".accum.f32", f.data(), f.size() * 4);
            write_file(*out + ".ids.u32", ids.data(), ids.size() * 4);
            write_file(*out + ".rgba8", rgba.data(), rgba.size());
            if (temporal) {
                const auto th = rs.temporal_history();
                const auto tf = rs.temporal_frame(dn_levels, dn_sigma_l, dn_sigma_z);
                const auto trgba = rs.temporal_rgba8(dn_levels, dn_sigma_l, dn_sigma_z);
                write_file(*out + ".temporal.f32", th.color.data(), th.color.size() * 4);
                write_file(*out + ".temporal.len.u32", th.length.data(), th.length.size() * 4);
                write_file(*out + ".temporal.denoised.f32", tf.data(), tf.size() * 4);
                write_file(*out + ".temporal.denoised.rgba8", trgba.data(), trgba.size());
            }
            if (denoise && !temporal) {
                const auto df = rs.denoise(dn_levels, dn_sigma_l, dn_sigma_z);
                const auto drgba = rs.denoised_rgba8(dn_levels, dn_sigma_l, dn_sigma_z);
                write_file(*out + ".denoised.f32", df.data(), df.size() * 4);
                write_file(*out + ".denoised.rgba8", drgba.data(), drgba.size());
            }
        }
        std::printf("{\"scene\":%s,\"mode\":%s,\"width\":%u,\"height\":%u,\"iteration\":%u,\"frames\":%u,"
                    "\"last_launch\":{\"samples\":%llu,\"primary\":%llu,\"shadow\":%llu,\"bounce\":%llu},\"camera\":%s%s}\n",
                    jstr(rs.scene().name).c_str(), jstr(mode_name(rs.mode())).c_str(), rs.width(), rs.height(),
                    rs.iteration(), frames, (unsigned long long)c.samples, (unsigned long long)c.primary,
                    (unsigned long long)c.shadow, (unsigned long long)c.bounce, cam_json(rs.camera()).c_str(),
                    noise_json.c_str());
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "rt_render: error %d: %s\n", e.code, e.what());
        return 1;
    }
}
