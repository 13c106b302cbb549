// Runs host/env_cdf.h and the CDF sampling of host/image_texture.h on the host
// for tests/test_env_cdf.py.
//   build <in> <out>: in = int32 width, height, compensate; float rgb[3 w h];
//                     out = the table, (h + w h) floats
//   sample <in> <out>: in = int32 width, height, n; float table[h + w h]; float u[2 n];
//                      out = per sample float x, y, pdf, pdf_continuous(x, y)
#include "env_cdf.h"

#include <cstdio>
#include <cstring>
#include <vector>

static bool read_all(const char* path, std::vector<char>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    std::vector<char> in;
    if (!read_all(argv[2], in) || in.size() < 12) return 3;
    int32_t head[3];
    std::memcpy(head, in.data(), 12);
    const int w = head[0], h = head[1];
    std::vector<float> out;
    if (!std::strcmp(argv[1], "build")) {
        if (in.size() != 12 + (size_t)w * h * 12) return 4;
        std::vector<float> rgb((size_t)w * h * 3);
        std::memcpy(rgb.data(), in.data() + 12, rgb.size() * 4);
        igx::build_env_cdf(rgb.data(), w, h, true, head[2] != 0, out);
    } else {
        const int n = head[2];
        const size_t cells = (size_t)h + (size_t)w * h;
        if (in.size() != 12 + cells * 4 + (size_t)n * 8) return 4;
        std::vector<float> table(cells), u(2 * (size_t)n);
        std::memcpy(table.data(), in.data() + 12, cells * 4);
        std::memcpy(u.data(), in.data() + 12 + cells * 4, u.size() * 4);
        out.resize(4 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            float x, y, pdf;
            igxd::cdf2d_sample_continuous(table.data(), w, h, u[2 * i], u[2 * i + 1], x, y, pdf);
            out[4 * i] = x;
            out[4 * i + 1] = y;
            out[4 * i + 2] = pdf;
            out[4 * i + 3] = igxd::cdf2d_pdf_continuous(table.data(), w, h, x, y);
        }
    }
    FILE* o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) return 5;
    std::fclose(o);
    std::puts("ok");
    return 0;
}
