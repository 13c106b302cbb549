// Evaluates host/image_texture.h on the host for tests/test_image_texture.py.
// Input file: int32 width, height, format, filter, wrap_u, wrap_v, n; float
// transform[6]; the texels (width * height * 4, 1 or 16 bytes); float uv[2 n].
// Output file: float rgba[4 n], the texture at every transformed uv.
#include "image_texture.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace igxd;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t head[7];
    float m[6];
    if (std::fread(head, 4, 7, in) != 7 || std::fread(m, 4, 6, in) != 6) return 4;
    const int w = head[0], h = head[1], format = head[2], filter = head[3], wu = head[4], wv = head[5], n = head[6];
    const size_t bytes = (size_t)w * h * (format == TEX_FLOAT4 ? 16 : format == TEX_MONO8 ? 1 : 4);
    std::vector<float> texels((bytes + 3) / 4 + 4); // float storage: 16-B aligned enough for the FLOAT4 loads below
    void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(texels.data()) + 15) & ~(uintptr_t)15);
    std::vector<float> uv(2 * (size_t)n), out(4 * (size_t)n);
    if (std::fread(base, 1, bytes, in) != bytes || std::fread(uv.data(), 4, uv.size(), in) != uv.size()) return 5;
    std::fclose(in);
    for (int i = 0; i < n; ++i) {
        float tu, tv;
        tex_transform(m, uv[2 * i], uv[2 * i + 1], tu, tv);
        const Texel c = tex_filter(filter, wu, wv, w, h, tu, tv, [&](int x, int y) {
            if (x < 0 || y < 0 || x >= w || y >= h) std::abort(); // a border rule left the image
            return tex_fetch(format, base, w, x, y);
        });
        out[4 * i] = c.r;
        out[4 * i + 1] = c.g;
        out[4 * i + 2] = c.b;
        out[4 * i + 3] = c.a;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) return 6;
    std::fclose(o);
    std::puts("ok");
    return 0;
}
