// Host evaluation of the shared camera and sky arithmetic (host/camera_model.h,
// host/cie_sky.h: the functions the kernels call), for tests/test_daylight.py,
// which compares the output with its float64 restatement.
//   daylight_check camera <20 camera numbers> <in> <out>
//       numbers: type width height eye[3] dir[3] up[3] fov vertical_fov aspect
//                near far ortho_scale aperture_radius focal_length
//       in: n x (nx, ny, u, v) float32; out: n x (org[3], dir[3]) float32
//   daylight_check sky <26 sky numbers> <in> <out>
//       numbers: kind has_ground zenith[3] ground[3] scale[3] ground_brightness
//                sun[3] zenith_ratio c2 transform[9] (row-major)
//       in: n x dir[3] float32 (local, Y up); out: n x rgb float32
#include "camera_model.h"
#include "cie_sky.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<float> read_floats(const char* path) {
    std::vector<float> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    float buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}
static void write_floats(const char* path, const std::vector<float>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fprintf(stderr, "cannot write %s\n", path); std::exit(2); }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    auto num = [&](int i) { return std::strtof(argv[2 + i], nullptr); };
    if (mode == "camera" && argc == 2 + 20 + 2) {
        igx_camera c{};
        c.type = (int)num(0);
        const int w = (int)num(1), h = (int)num(2);
        for (int i = 0; i < 3; ++i) { c.eye[i] = num(3 + i); c.dir[i] = num(6 + i); c.up[i] = num(9 + i); }
        c.fov = num(12);
        c.vertical_fov = (int)num(13);
        c.aspect = num(14);
        c.near_clip = num(15);
        c.far_clip = num(16);
        c.ortho_scale = num(17);
        c.aperture_radius = num(18);
        c.focal_length = num(19);
        const igxd::CameraModel k = igxd::make_camera_model(c, w, h);
        const std::vector<float> in = read_floats(argv[2 + 20]);
        std::vector<float> out;
        for (size_t i = 0; i + 3 < in.size(); i += 4) {
            igxd::CamVec o, d;
            igxd::camera_ray(k.cam, k.lens, in[i], in[i + 1], in[i + 2], in[i + 3], o, d);
            const float r[6] = {o.x, o.y, o.z, d.x, d.y, d.z};
            out.insert(out.end(), r, r + 6);
        }
        write_floats(argv[2 + 21], out);
        std::printf("ok\n");
        return 0;
    }
    if (mode == "sky" && argc == 2 + 26 + 2) {
        igx_light L{};
        L.type = IGX_LIGHT_CIE;
        L.sky_kind = (int)num(0);
        L.has_ground = (int)num(1);
        for (int i = 0; i < 3; ++i) { L.sky_zenith[i] = num(2 + i); L.sky_ground[i] = num(5 + i); L.sky_scale[i] = num(8 + i); L.sun_direction[i] = num(12 + i); }
        L.ground_brightness = num(11);
        L.zenith_ratio = num(15);
        L.sky_c2 = num(16);
        for (int i = 0; i < 9; ++i) L.sky_transform[i] = num(17 + i);
        const igxd::CieSky sky = igxd::make_cie_sky(L);
        const std::vector<float> in = read_floats(argv[2 + 26]);
        std::vector<float> out;
        for (size_t i = 0; i + 2 < in.size(); i += 3) {
            const igxd::SkyVec e = igxd::cie_sky_radiance(sky, igxd::SkyVec{in[i], in[i + 1], in[i + 2]});
            const float r[3] = {e.x, e.y, e.z};
            out.insert(out.end(), r, r + 3);
        }
        write_floats(argv[2 + 27], out);
        std::printf("ok\n");
        return 0;
    }
    std::fprintf(stderr, "usage: daylight_check camera|sky <numbers> <in> <out>\n");
    return 2;
}
