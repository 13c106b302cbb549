// igcli-style frontend over the HIP device (src/frontend/cli/main.cpp:54-179):
// loads a scene, renders spp samples in iterations of spi on one GPU (or
// iterations until --time seconds of rendering, main.cpp:138), prints
// Msamples/s like the reference (cli/main.cpp:135, 172-178) plus Mrays/s, and
// writes the averaged image as EXR (Image::save, Image.h:92-101), or PFM when
// the output name ends in .pfm.  The scene reaches the device as the
// reference's does: the loader's tables (SceneDatabase, serialize_scene) go
// through IG::Device::assignScene, the shading tables through render's shader
// set (Runtime.cpp:477-485, 343).  --eye / --dir / --up override the scene
// camera's orientation the way Runtime::setCameraOrientationParameter does
// (main.cpp:103-107, Runtime.cpp:703-708): as the __camera_* vector
// parameters of render's ParameterSet.  --width / --height override the film
// (ProgramOptions.cpp:135-139).  --stats prints Statistics::dump's quantities
// (main.cpp:155-166).  --denoise-aovs enables the denoiser's feature buffers
// (RuntimeOptions::Denoiser without the denoiser network itself): the info-buffer
// pass fills "Normals", "Albedo" and "Depth" in the first iteration, or in every
// one with --denoiser-aov-every-iteration; --denoiser-follow-specular as the
// reference's flag (ProgramOptions.cpp:211-213); -o then writes one EXR with
// the layers Default / Normals / Albedo / Depth, each over its own iteration
// count (frontend/common/IO.cpp:72-129).  --imageinfo [BINS] prints one line
// `imageinfo {json}` with the film's luminance statistics (and with BINS the
// four histograms), --ppm FILE [--tonemap N] [--gamma] writes the tonemapped
// film as a binary PPM; both run on the device (Device::imageinfo /
// Device::tonemap).  --glare [--glare-mul M] [--glare-ev E] prints one line
// `glare: dgp D ev E avg_lum L omega O pixels N`: the daylight glare probability
// of the film through the scene's camera (Device::evaluateGlare), with the
// threshold M (default 5) times imageinfo's average, the colour ramp up to its
// soft maximum, as the viewer calls it (UI.cpp:651), and the vertical
// illuminance computed unless E is given; with --ppm the heat map of the glare
// source lies over the tonemapped image.  Options of the reference's other
// targets and of its shader compiler are refused with a message.
#include "Device.h"
#include "igx_scene.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static void usage() {
    std::fprintf(stderr,
                 "usage: igcli SCENE.json [--spp N | --time SECONDS] [--spi N] [--seed N] [--gpu] [--gpu-device N]\n"
                 "             [--width W --height H] [--eye X Y Z] [--dir X Y Z] [--up X Y Z] [--stats]\n"
                 "             [--denoise-aovs [--denoiser-aov-every-iteration] [--denoiser-follow-specular]]\n"
                 "             [--imageinfo [BINS]] [--ppm out.ppm [--tonemap 0..4] [--gamma]]\n"
                 "             [--glare [--glare-mul M] [--glare-ev E]]\n"
                 "             [-o out.exr|out.pfm]\n");
}

int main(int argc, char** argv) {
    std::string scene_path, out_path;
    int spp = 0, spi = 8, seed = 0, device = 0, width = 0, height = 0;
    double render_time = 0; // --time: seconds of rendering instead of a sample count
    bool stats = false;
    int info_bins = -1; // --imageinfo: -1 off, 0 statistics only, n > 0 with histograms of n bins
    std::string ppm_path;
    int tonemap_method = 0;
    bool tonemap_gamma = false;
    bool glare = false;
    float glare_mul = 5.0f, glare_ev = -1.0f; // --glare-ev: < 0 = computed
    IG::Device::DenoiserSettings denoiser;
    IG::ParameterSet params; // the camera orientation overrides (__camera_eye / _dir / _up)
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { usage(); std::exit(2); }
            return argv[++i];
        };
        auto vec3 = [&](const char* key) {
            IG::Vector3f v;
            for (int k = 0; k < 3; ++k) {
                const char* t = next();
                char* end = nullptr;
                v[k] = std::strtof(t, &end);
                if (end == t || *end) { std::fprintf(stderr, "igcli: %s needs three numbers\n", a.c_str()); std::exit(2); }
            }
            params.VectorParameters[key] = v;
        };
        if (a == "--spp") spp = std::atoi(next());
        else if (a == "--spi") spi = std::atoi(next());
        else if (a == "--seed") seed = std::atoi(next());
        else if (a == "--gpu-device") device = std::atoi(next());
        else if (a == "--time") render_time = std::atof(next());
        else if (a == "--width") width = std::atoi(next());
        else if (a == "--height") height = std::atoi(next());
        else if (a == "--eye") vec3("__camera_eye");
        else if (a == "--dir") vec3("__camera_dir");
        else if (a == "--up") vec3("__camera_up");
        else if (a == "--stats" || a == "--stats-full") stats = true;
        else if (a == "--denoise-aovs") denoiser.Enabled = true;
        else if (a == "--denoiser-aov-every-iteration") denoiser.OnlyFirstIteration = false;
        else if (a == "--denoiser-aov-first-iteration") denoiser.OnlyFirstIteration = true;
        else if (a == "--denoiser-follow-specular") denoiser.FollowSpecular = true;
        else if (a == "--denoiser-skip-specular") denoiser.FollowSpecular = false;
        else if (a == "--imageinfo") {
            info_bins = 0;
            if (i + 1 < argc && argv[i + 1][0] && std::strspn(argv[i + 1], "0123456789") == std::strlen(argv[i + 1]))
                info_bins = std::atoi(argv[++i]);
        }
        else if (a == "--ppm") ppm_path = next();
        else if (a == "--tonemap") tonemap_method = std::atoi(next());
        else if (a == "--gamma") tonemap_gamma = true;
        else if (a == "--glare") glare = true;
        else if (a == "--glare-mul") glare_mul = (float)std::atof(next());
        else if (a == "--glare-ev") glare_ev = (float)std::atof(next());
        else if (a == "-o" || a == "--output") out_path = next();
        else if (a == "--gpu" || a == "--no-progress" || a == "--no-color" || a == "-q" || a == "--quiet") {}
        else if (a == "--cpu" || a == "--cpu-arch" || a == "--cpu-threads" || a == "--cpu-vectorwidth") {
            std::fprintf(stderr, "igcli: %s: this build's device is GPU-only (igx, HIP on gfx950); the reference's CPU "
                                 "device is not part of it\n", a.c_str());
            return 2;
        }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (!a.empty() && a[0] == '-') {
            std::fprintf(stderr, "igcli: unknown option %s\n", a.c_str());
            usage();
            return 2;
        }
        else scene_path = a;
    }
    if (spp > 0 && render_time > 0) { std::fprintf(stderr, "igcli: --time excludes --spp\n"); return 2; }
    if ((width > 0) != (height > 0)) { std::fprintf(stderr, "igcli: --width needs --height and vice versa\n"); return 2; }
    if (spi < 1) { std::fprintf(stderr, "igcli: --spi must be positive\n"); return 2; }
    if (scene_path.empty()) { usage(); return 2; }
    char err[1024] = {0};
    igx_scene* scene = igx_scene_load_file(scene_path.c_str(), err, sizeof(err));
    if (!scene) { std::fprintf(stderr, "failed to load scene: %s\n", err); return 1; }
    const igx_scene_desc* desc = igx_scene_get_desc(scene);
    if (spp <= 0) spp = spi;
    // igcli rounds spp up to a multiple of spi (cli/main.cpp:110-113); with
    // --time the loop runs until that much rendering time has passed
    const int iters = render_time > 0 ? 0 : (spp + spi - 1) / spi;
    const int W = width > 0 ? width : desc->film_width, H = height > 0 ? height : desc->film_height;
    try {
        IG::SceneDatabase db;
        IG::TechniqueVariantShaderSet shaders;
        IG::serialize_scene(*desc, db, shaders.shading);
        shaders.GlareEnabled = glare;
        IG::Device::SetupSettings ss;
        ss.target = IG::Target::makeGPU(device);
        ss.AcquireStats = stats;
        IG::Device dev(ss);
        if (denoiser.Enabled) dev.setDenoiser(denoiser);
        IG::Device::SceneSettings sc;
        sc.database = &db;
        dev.assignScene(sc);
        std::vector<double> rates;
        double total_s = 0; // wall time of the render loop (cli/main.cpp:127-135)
        const auto t_all = std::chrono::steady_clock::now();
        for (int it = 0; render_time > 0 ? total_s < render_time : it < iters; ++it) {
            IG::Device::RenderSettings rs;
            rs.spi = spi;
            rs.width = W;
            rs.height = H;
            rs.iteration = it;
            rs.user_seed = seed;
            auto t0 = std::chrono::steady_clock::now();
            dev.render(shaders, rs, params.empty() ? nullptr : &params);
            dev.synchronize(); // render() only queues the iteration
            double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            rates.push_back((double)spi * W * H / s / 1e6);
            total_s += s;
        }
        const igx_stats& st = dev.getStatistics()->raw();
        std::sort(rates.begin(), rates.end());
        double rays = (double)(st.camera_rays + st.bounce_rays + st.shadow_rays);
        std::printf("# %f %f %f Msamples/s\n", rates.front(), rates[rates.size() / 2], rates.back());
        std::printf("# %.3f Mrays/s (camera %llu, bounce %llu, shadow %llu) over %.3f ms\n", rays / total_s / 1e6,
                    (unsigned long long)st.camera_rays, (unsigned long long)st.bounce_rays, (unsigned long long)st.shadow_rays,
                    total_s * 1e3);
        if (stats) {
            const size_t all_ms = (size_t)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count());
            std::printf("%s  Iterations: %zu\n  SPP: %zu\n  SPI: %d\n", dev.getStatistics()->dump(all_ms, rates.size()).c_str(),
                        rates.size(), rates.size() * (size_t)spi, spi);
        }
        if (info_bins >= 0) {
            std::vector<int> hist[4];
            for (auto& h : hist) h.assign((size_t)std::max(info_bins, 1), 0);
            const IG::ImageInfoSettings is{"", 1.0f, (size_t)info_bins, hist[0].data(), hist[1].data(), hist[2].data(), hist[3].data(),
                                           true, info_bins > 0};
            const IG::ImageInfoOutput io = dev.imageinfo(is);
            // %.9g round-trips a float
            std::printf("imageinfo {\"min\": %.9g, \"max\": %.9g, \"avg\": %.9g, \"soft_min\": %.9g, \"soft_max\": %.9g, "
                        "\"median\": %.9g, \"inf_count\": %d, \"nan_count\": %d, \"neg_count\": %d",
                        io.Min, io.Max, io.Average, io.SoftMin, io.SoftMax, io.Median, io.InfCount, io.NaNCount, io.NegCount);
            const char* names[4] = {"histogram_r", "histogram_g", "histogram_b", "histogram_l"};
            for (int c = 0; c < 4 && info_bins > 0; ++c) {
                std::printf(", \"%s\": [", names[c]);
                for (int k = 0; k < info_bins; ++k) std::printf(k ? ", %d" : "%d", hist[c][k]);
                std::printf("]");
            }
            std::printf("}\n");
        }
        std::vector<uint32_t> px;
        if (!ppm_path.empty()) {
            px.assign((size_t)W * H, 0xff000000u);
            dev.tonemap(px.data(), IG::TonemapSettings{"", (size_t)tonemap_method, tonemap_gamma, 1.0f, 1.0f, 0.0f});
        }
        if (glare) {
            const IG::ImageInfoOutput io = dev.imageinfo(IG::ImageInfoSettings{"", 1.0f, 0, nullptr, nullptr, nullptr, nullptr, false, false});
            const IG::GlareOutput g = dev.evaluateGlare(px.empty() ? nullptr : px.data(),
                                                        IG::GlareSettings{"", 1.0f, io.SoftMax, io.Average, glare_mul, glare_ev});
            std::printf("glare: dgp %.9g ev %.9g avg_lum %.9g omega %.9g pixels %d\n", g.DGP, g.VerticalIlluminance, g.AvgLum, g.AvgOmega,
                        g.NumPixels);
        }
        if (!ppm_path.empty()) {
            FILE* f = std::fopen(ppm_path.c_str(), "wb");
            if (!f) { std::fprintf(stderr, "cannot write %s\n", ppm_path.c_str()); return 1; }
            std::fprintf(f, "P6\n%d %d\n255\n", W, H);
            std::vector<unsigned char> row(3 * (size_t)W);
            for (int y = 0; y < H; ++y) {
                for (int x = 0; x < W; ++x) {
                    const uint32_t p = px[(size_t)y * W + x];
                    row[3 * x] = (unsigned char)(p >> 16), row[3 * x + 1] = (unsigned char)(p >> 8), row[3 * x + 2] = (unsigned char)p;
                }
                std::fwrite(row.data(), 1, row.size(), f);
            }
            std::fclose(f);
        }
        if (!out_path.empty()) {
            IG::Device::AOVAccessor acc = dev.getFramebufferForHost("");
            float inv = acc.IterationCount ? 1.0f / acc.IterationCount : 0.0f;
            const bool pfm = out_path.size() >= 4 && out_path.compare(out_path.size() - 4, 4, ".pfm") == 0;
            if (!pfm && denoiser.Enabled) {
                // the film as "Default" and the three AOVs, each over its own count (IO.cpp:72-129)
                const char* names[4] = {"Default", "Normals", "Albedo", "Depth"};
                const float* planes[4] = {acc.Data, nullptr, nullptr, nullptr};
                float scales[4] = {inv, 0, 0, 0};
                for (int k = 1; k < 4; ++k) {
                    IG::Device::AOVAccessor aov = dev.getFramebufferForHost(names[k]);
                    planes[k] = aov.Data;
                    scales[k] = aov.IterationCount ? 1.0f / aov.IterationCount : 0.0f;
                }
                if (igx_write_exr_layers(out_path.c_str(), names, planes, 4, W, H, scales) != 0) {
                    std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
                    return 1;
                }
            } else if (!pfm) {
                if (igx_write_exr(out_path.c_str(), acc.Data, W, H, 3, inv) != 0) {
                    std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
                    return 1;
                }
            } else {
                FILE* f = std::fopen(out_path.c_str(), "wb");
                if (!f) { std::fprintf(stderr, "cannot write %s\n", out_path.c_str()); return 1; }
                std::fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
                for (int y = H - 1; y >= 0; --y) { // PFM rows go bottom-up
                    std::vector<float> row(3 * W);
                    for (int x = 0; x < 3 * W; ++x) row[x] = acc.Data[(size_t)y * 3 * W + x] * inv;
                    std::fwrite(row.data(), sizeof(float), row.size(), f);
                }
                std::fclose(f);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        igx_scene_free(scene);
        return 1;
    }
    igx_scene_free(scene);
    return 0;
}
