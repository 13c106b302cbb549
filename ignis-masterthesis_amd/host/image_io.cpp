// PNG / OpenEXR / Radiance readers of image textures (host/image_io.h).
#include "image_io.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>

namespace igx {
namespace {

struct Reason {
    std::string text;
};
[[noreturn]] void refuse(const std::string& why) { throw Reason{why}; }

// ---- inflate (RFC 1951) -----------------------------------------------------
struct BitReader {
    const uint8_t* p;
    size_t n, pos = 0;
    uint32_t buf = 0;
    int cnt = 0;
    uint32_t bits(int k) {
        while (cnt < k) {
            if (pos >= n) refuse("truncated deflate stream");
            buf |= (uint32_t)p[pos++] << cnt;
            cnt += 8;
        }
        const uint32_t v = buf & ((1u << k) - 1u);
        buf >>= k;
        cnt -= k;
        return v;
    }
    void align_byte() {
        buf = 0;
        cnt = 0;
    }
};

// canonical Huffman code: symbols ordered by (length, value)
struct Huffman {
    uint16_t count[16];
    uint16_t symbol[288];
    // false for an over-subscribed set of lengths; `complete` tells a full code
    bool build(const uint8_t* len, int n, bool& complete) {
        std::memset(count, 0, sizeof(count));
        for (int i = 0; i < n; ++i) ++count[len[i]];
        int left = 1;
        for (int l = 1; l < 16; ++l) {
            left = left * 2 - count[l];
            if (left < 0) return false;
        }
        complete = left == 0;
        uint16_t offs[16];
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        for (int i = 0; i < n; ++i)
            if (len[i]) symbol[offs[len[i]]++] = (uint16_t)i;
        return true;
    }
    int decode(BitReader& br) const {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; ++l) {
            code |= (int)br.bits(1);
            const int c = count[l];
            if (code - c < first) return symbol[index + (code - first)];
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        refuse("invalid Huffman code in deflate stream");
    }
};

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

void inflate_codes(BitReader& br, const Huffman& lit, const Huffman& dist, std::vector<uint8_t>& out, size_t limit) {
    for (;;) {
        const int s = lit.decode(br);
        if (s < 256) {
            if (out.size() >= limit) refuse("deflate stream longer than the image");
            out.push_back((uint8_t)s);
        } else if (s == 256) {
            return;
        } else {
            if (s > 285) refuse("invalid length symbol in deflate stream");
            const size_t len = kLenBase[s - 257] + br.bits(kLenExtra[s - 257]);
            const int ds = dist.decode(br);
            if (ds > 29) refuse("invalid distance symbol in deflate stream");
            const size_t d = kDistBase[ds] + br.bits(kDistExtra[ds]);
            if (d > out.size()) refuse("deflate distance reaches before the stream");
            if (out.size() + len > limit) refuse("deflate stream longer than the image");
            size_t from = out.size() - d;
            for (size_t k = 0; k < len; ++k) out.push_back(out[from + k]);
        }
    }
}

void inflate_raw(BitReader& br, std::vector<uint8_t>& out, size_t limit) {
    for (;;) {
        const uint32_t last = br.bits(1), type = br.bits(2);
        if (type == 0) {
            br.align_byte();
            if (br.pos + 4 > br.n) refuse("truncated deflate stream");
            const uint32_t len = br.p[br.pos] | (br.p[br.pos + 1] << 8), nlen = br.p[br.pos + 2] | (br.p[br.pos + 3] << 8);
            br.pos += 4;
            if ((len ^ 0xffffu) != nlen) refuse("corrupt stored block in deflate stream");
            if (br.pos + len > br.n) refuse("truncated deflate stream");
            if (out.size() + len > limit) refuse("deflate stream longer than the image");
            out.insert(out.end(), br.p + br.pos, br.p + br.pos + len);
            br.pos += len;
        } else if (type == 1) {
            uint8_t len[288 + 30];
            for (int i = 0; i < 144; ++i) len[i] = 8;
            for (int i = 144; i < 256; ++i) len[i] = 9;
            for (int i = 256; i < 280; ++i) len[i] = 7;
            for (int i = 280; i < 288; ++i) len[i] = 8;
            for (int i = 0; i < 30; ++i) len[288 + i] = 5;
            Huffman lit, dist;
            bool c;
            lit.build(len, 288, c);
            dist.build(len + 288, 30, c);
            inflate_codes(br, lit, dist, out, limit);
        } else if (type == 2) {
            const int nlen = (int)br.bits(5) + 257, ndist = (int)br.bits(5) + 1, ncode = (int)br.bits(4) + 4;
            if (nlen > 286 || ndist > 30) refuse("invalid code counts in deflate stream");
            static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t len[286 + 30] = {};
            uint8_t cl[19] = {};
            for (int i = 0; i < ncode; ++i) cl[order[i]] = (uint8_t)br.bits(3);
            Huffman lencode;
            bool complete;
            if (!lencode.build(cl, 19, complete) || !complete) refuse("invalid code-length code in deflate stream");
            int i = 0;
            while (i < nlen + ndist) {
                const int s = lencode.decode(br);
                if (s < 16) {
                    len[i++] = (uint8_t)s;
                } else {
                    uint8_t v = 0;
                    int rep;
                    if (s == 16) {
                        if (i == 0) refuse("deflate length repeat without a length");
                        v = len[i - 1];
                        rep = 3 + (int)br.bits(2);
                    } else if (s == 17) {
                        rep = 3 + (int)br.bits(3);
                    } else {
                        rep = 11 + (int)br.bits(7);
                    }
                    if (i + rep > nlen + ndist) refuse("deflate length repeat past the code");
                    while (rep--) len[i++] = v;
                }
            }
            if (len[256] == 0) refuse("deflate block without an end code");
            Huffman lit, dist;
            // an incomplete code is allowed only where it has a single symbol
            if (!lit.build(len, nlen, complete) || (!complete && nlen != lit.count[0] + lit.count[1]))
                refuse("invalid literal code in deflate stream");
            if (!dist.build(len + nlen, ndist, complete) || (!complete && ndist != dist.count[0] + dist.count[1]))
                refuse("invalid distance code in deflate stream");
            inflate_codes(br, lit, dist, out, limit);
        } else {
            refuse("invalid block type in deflate stream");
        }
        if (last) return;
    }
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

std::vector<uint8_t> zlib_inflate_or_refuse(const uint8_t* data, size_t n, size_t expected) {
    if (n < 6) refuse("truncated zlib stream");
    if ((data[0] & 0x0f) != 8 || (data[0] >> 4) > 7 || ((data[0] << 8) | data[1]) % 31 != 0 || (data[1] & 0x20))
        refuse("invalid zlib header");
    BitReader br{data + 2, n - 2};
    std::vector<uint8_t> out;
    // deflate expands at most 1032 : 1 (a 258-byte match from two bits): a stream too short for the
    // image is refused before any buffer of the image's size exists
    if (expected / 1032 > n) refuse("zlib stream too short for the image");
    out.reserve(expected);
    inflate_raw(br, out, expected);
    if (out.size() != expected) refuse("zlib stream shorter than the image");
    if (br.pos + 4 > br.n) refuse("truncated zlib stream");
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < out.size();) {
        const size_t end = std::min(out.size(), i + 5552);
        for (; i < end; ++i) {
            a += out[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
    }
    if (be32(br.p + br.pos) != ((b << 16) | a)) refuse("zlib checksum mismatch");
    return out;
}

void check_size(int64_t w, int64_t h) {
    if (w < 1 || h < 1) refuse("empty image");
    if (w > MAX_IMAGE_SIDE || h > MAX_IMAGE_SIDE)
        refuse("image of " + std::to_string(w) + " x " + std::to_string(h) + " exceeds the largest side of " + std::to_string(MAX_IMAGE_SIDE));
}

// ---- PNG ----------------------------------------------------------------------
struct CrcTable {
    uint32_t entry[256];
    constexpr CrcTable() : entry() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            entry[i] = c;
        }
    }
};
constexpr CrcTable kCrcTable; // built by the compiler: nothing to initialise when two scenes load at once

uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) c = kCrcTable.entry[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

LoadedImage read_png(const uint8_t* d, size_t n, bool linear) {
    size_t pos = 8;
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = -1;
    bool have_ihdr = false, have_end = false;
    std::vector<uint8_t> idat, plte, trns;
    while (!have_end) {
        if (pos + 12 > n) refuse("truncated PNG (chunk header)");
        const uint32_t len = be32(d + pos);
        if (len > n || pos + 12 + (size_t)len > n) refuse("truncated PNG (chunk data)");
        const uint8_t* tag = d + pos + 4;
        const uint8_t* body = d + pos + 8;
        if (crc32_of(tag, 4 + (size_t)len) != be32(body + len)) refuse("corrupt PNG (chunk CRC mismatch)");
        const bool is = !have_ihdr;
        if (is && std::memcmp(tag, "IHDR", 4) != 0) refuse("corrupt PNG (no IHDR first)");
        if (!std::memcmp(tag, "IHDR", 4)) {
            if (have_ihdr || len != 13) refuse("corrupt PNG (IHDR)");
            have_ihdr = true;
            w = be32(body);
            h = be32(body + 4);
            depth = body[8];
            ctype = body[9];
            if ((w | h) & 0x80000000u) refuse("corrupt PNG (size)");
            check_size(w, h);
            if (body[10] != 0 || body[11] != 0) refuse("corrupt PNG (compression or filter method)");
            if (body[12] == 1) refuse("interlaced PNG is not supported");
            if (body[12] != 0) refuse("corrupt PNG (interlace method)");
            const bool ok = (ctype == 0 && (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)) ||
                            (ctype == 3 && (depth == 1 || depth == 2 || depth == 4 || depth == 8)) ||
                            ((ctype == 2 || ctype == 4 || ctype == 6) && (depth == 8 || depth == 16));
            if (!ok) refuse("corrupt PNG (colour type " + std::to_string(ctype) + " with bit depth " + std::to_string(depth) + ")");
        } else if (!std::memcmp(tag, "PLTE", 4)) {
            if (len % 3 != 0 || len > 768 || len == 0) refuse("corrupt PNG (PLTE)");
            plte.assign(body, body + len);
        } else if (!std::memcmp(tag, "tRNS", 4)) {
            trns.assign(body, body + len);
        } else if (!std::memcmp(tag, "IDAT", 4)) {
            idat.insert(idat.end(), body, body + len);
        } else if (!std::memcmp(tag, "IEND", 4)) {
            have_end = true;
        } else if (!(tag[0] & 0x20)) {
            refuse("PNG with an unknown critical chunk");
        }
        pos += 12 + (size_t)len;
    }
    if (!have_ihdr) refuse("corrupt PNG (no IHDR)");
    if (ctype == 3 && plte.empty()) refuse("corrupt PNG (palette image without PLTE)");
    const int comps = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
    const size_t bits_px = (size_t)comps * depth;
    const size_t row_bytes = ((size_t)w * bits_px + 7) / 8, bpp = std::max<size_t>(1, bits_px / 8);
    std::vector<uint8_t> raw = zlib_inflate_or_refuse(idat.data(), idat.size(), (size_t)h * (1 + row_bytes));
    // unfilter in place (PNG specification, section 9)
    for (uint32_t y = 0; y < h; ++y) {
        uint8_t* cur = raw.data() + (size_t)y * (1 + row_bytes) + 1;
        const uint8_t* up = y ? cur - (1 + row_bytes) : nullptr;
        const int filter = cur[-1];
        if (filter > 4) refuse("corrupt PNG (filter type " + std::to_string(filter) + ")");
        for (size_t x = 0; x < row_bytes; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int pred = 0;
            if (filter == 1) pred = a;
            else if (filter == 2) pred = b;
            else if (filter == 3) pred = (a + b) >> 1;
            else if (filter == 4) {
                const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            cur[x] = (uint8_t)(cur[x] + pred);
        }
    }
    // to 8-bit samples: channels as stb counts them (grey 1, grey+alpha 2, RGB 3, RGBA 4;
    // a palette 3, or 4 with tRNS)
    const bool mono = ctype == 0;
    LoadedImage img;
    img.width = (int32_t)w;
    img.height = (int32_t)h;
    img.format = mono ? IMAGE_MONO8 : IMAGE_RGBA8;
    img.pixels.resize((size_t)w * h * (mono ? 1 : 4));
    auto lin = [&](uint8_t c) { return linear ? c : byte_color_to_linear(c); };
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t* src = raw.data() + (size_t)y * (1 + row_bytes) + 1;
        uint8_t* dst = img.pixels.data() + (size_t)(h - 1 - y) * w * (mono ? 1 : 4);
        for (uint32_t x = 0; x < w; ++x) {
            auto sample = [&](int c) -> uint8_t { // component c of pixel x, reduced to 8 bit
                if (depth == 8) return src[(size_t)x * comps + c];
                if (depth == 16) return src[((size_t)x * comps + c) * 2];
                const size_t bit = (size_t)x * depth;
                return (uint8_t)((src[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1));
            };
            if (ctype == 0) {
                uint8_t g = sample(0);
                if (depth < 8) g = (uint8_t)(g * (255 / ((1 << depth) - 1)));
                dst[x] = lin(g);
            } else if (ctype == 3) {
                const size_t k = sample(0);
                if (k * 3 + 2 >= plte.size()) refuse("corrupt PNG (palette index out of range)");
                dst[4 * x + 0] = lin(plte[3 * k]);
                dst[4 * x + 1] = lin(plte[3 * k + 1]);
                dst[4 * x + 2] = lin(plte[3 * k + 2]);
                dst[4 * x + 3] = k < trns.size() ? trns[k] : 255;
            } else if (ctype == 4) {
                const uint8_t g = lin(sample(0));
                dst[4 * x + 0] = dst[4 * x + 1] = dst[4 * x + 2] = g;
                dst[4 * x + 3] = sample(1);
            } else {
                dst[4 * x + 0] = lin(sample(0));
                dst[4 * x + 1] = lin(sample(1));
                dst[4 * x + 2] = lin(sample(2));
                dst[4 * x + 3] = ctype == 6 ? sample(3) : 255;
            }
        }
    }
    return img;
}

// ---- OpenEXR --------------------------------------------------------------------
float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 0x1f, m = h & 0x3ff;
    uint32_t u;
    if (e == 0) {
        if (m == 0) {
            u = s;
        } else { // subnormal
            int sh = 0;
            uint32_t mm = m;
            while (!(mm & 0x400)) {
                mm <<= 1;
                ++sh;
            }
            u = s | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((mm & 0x3ff) << 13);
        }
    } else if (e == 31) {
        u = s | 0x7f800000u | (m << 13);
    } else {
        u = s | ((e + 127 - 15) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

LoadedImage read_exr(const uint8_t* d, size_t n) {
    if (n < 8) refuse("truncated EXR (header)");
    const uint32_t version = le32(d + 4);
    if ((version & 0xff) != 2) refuse("unsupported EXR version " + std::to_string(version & 0xff));
    if (version & 0x200) refuse("tiled EXR is not supported");
    if (version & 0x1000) refuse("multipart EXR is not supported");
    if (version & 0x800) refuse("deep EXR is not supported");
    size_t pos = 8;
    auto cstr = [&](size_t limit) {
        std::string s;
        for (;;) {
            if (pos >= n) refuse("truncated EXR (header)");
            const char c = (char)d[pos++];
            if (!c) return s;
            if (s.size() >= limit) refuse("corrupt EXR (name too long)");
            s += c;
        }
    };
    struct Channel {
        std::string name;
        int type; // 1 half, 2 float
    };
    std::vector<Channel> channels;
    int compression = -1;
    int64_t win[4] = {0, 0, -1, -1};
    bool have_win = false;
    for (;;) {
        const std::string name = cstr(255);
        if (name.empty()) break;
        const std::string type = cstr(255);
        if (pos + 4 > n) refuse("truncated EXR (header)");
        const uint32_t size = le32(d + pos);
        pos += 4;
        if (size > n || pos + size > n) refuse("truncated EXR (attribute " + name + ")");
        const uint8_t* a = d + pos;
        if (name == "channels") {
            if (type != "chlist") refuse("corrupt EXR (channels)");
            const size_t end = pos + size;
            size_t save = pos;
            for (;;) {
                const std::string cn = cstr(255);
                if (cn.empty()) break;
                if (pos + 16 > end) refuse("corrupt EXR (channel list)");
                const uint32_t pt = le32(d + pos), xs = le32(d + pos + 8), ys = le32(d + pos + 12);
                pos += 16;
                if (pt != 1 && pt != 2) refuse("EXR channel " + cn + " is neither half nor float");
                if (xs != 1 || ys != 1) refuse("subsampled EXR channels are not supported");
                channels.push_back({cn, (int)pt});
                if (channels.size() > 64) refuse("corrupt EXR (too many channels)");
            }
            if (pos > end) refuse("corrupt EXR (channel list)");
            pos = save;
        } else if (name == "compression") {
            if (size != 1) refuse("corrupt EXR (compression)");
            compression = a[0];
        } else if (name == "dataWindow") {
            if (size != 16) refuse("corrupt EXR (dataWindow)");
            for (int k = 0; k < 4; ++k) win[k] = (int32_t)le32(a + 4 * k);
            have_win = true;
        } else if (name == "tiles") {
            refuse("tiled EXR is not supported");
        }
        pos += size;
    }
    if (channels.empty() || compression < 0 || !have_win) refuse("corrupt EXR (header lacks channels, compression or dataWindow)");
    static const char* const kComp[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
    if (compression != 0 && compression != 2 && compression != 3)
        refuse(std::string("EXR compression ") + (compression < 10 ? kComp[compression] : "?") + " is not supported (NONE, ZIPS and ZIP are)");
    const int64_t w = win[2] - win[0] + 1, h = win[3] - win[1] + 1;
    check_size(w, h);
    // where each file channel goes in RGBA
    std::vector<int> slot(channels.size(), -1);
    bool has[4] = {false, false, false, false}, has_y = false;
    size_t line_bytes = 0;
    for (size_t c = 0; c < channels.size(); ++c) {
        const std::string& cn = channels[c].name;
        if (cn == "R") slot[c] = 0;
        else if (cn == "G") slot[c] = 1;
        else if (cn == "B") slot[c] = 2;
        else if (cn == "A") slot[c] = 3;
        else if (cn == "Y") slot[c] = 4;
        if (slot[c] >= 0 && slot[c] < 4) has[slot[c]] = true;
        if (slot[c] == 4) has_y = true;
        line_bytes += (size_t)w * (channels[c].type == 1 ? 2 : 4);
    }
    const bool rgb = has[0] && has[1] && has[2];
    if (!rgb && !has_y) refuse("EXR without the channels R G B or Y");
    const int lines_per_chunk = compression == 3 ? 16 : 1;
    const size_t n_chunks = ((size_t)h + lines_per_chunk - 1) / lines_per_chunk;
    if (pos + n_chunks * 8 > n) refuse("truncated EXR (offset table)");
    // the file must be able to hold the image before a buffer of its size exists: raw lines as
    // they are, compressed ones at deflate's best ratio of 1032 : 1
    {
        const size_t raw_total = line_bytes * (size_t)h, rest = n - pos - n_chunks * 8;
        if ((compression == 0 ? raw_total : raw_total / 1032) > rest) refuse("truncated EXR (file too short for the image)");
    }
    LoadedImage img;
    img.width = (int32_t)w;
    img.height = (int32_t)h;
    img.format = IMAGE_FLOAT4;
    img.pixels.resize((size_t)w * h * 16);
    float* px = reinterpret_cast<float*>(img.pixels.data());
    for (size_t i = 0; i < (size_t)w * h; ++i) px[4 * i + 3] = 1.0f;
    std::vector<uint8_t> seen(n_chunks, 0), tmp;
    for (size_t k = 0; k < n_chunks; ++k) {
        const uint64_t off = le64(d + pos + 8 * k);
        if (off > n || off + 8 > n) refuse("truncated EXR (chunk " + std::to_string(k) + ")");
        const int64_t y0 = (int32_t)le32(d + off) - win[1];
        const uint32_t size = le32(d + off + 4);
        if (size > n || off + 8 + size > n) refuse("truncated EXR (chunk " + std::to_string(k) + ")");
        if (y0 < 0 || y0 >= h || y0 % lines_per_chunk != 0 || seen[(size_t)y0 / lines_per_chunk]) refuse("corrupt EXR (chunk line)");
        seen[(size_t)y0 / lines_per_chunk] = 1;
        const int lines = (int)std::min<int64_t>(lines_per_chunk, h - y0);
        const size_t raw_bytes = line_bytes * lines;
        const uint8_t* data = d + off + 8;
        if (compression != 0 && size < raw_bytes) {
            std::vector<uint8_t> z = zlib_inflate_or_refuse(data, size, raw_bytes);
            // undo the predictor, then the split into even and odd bytes
            for (size_t i = 1; i < raw_bytes; ++i) z[i] = (uint8_t)(z[i - 1] + z[i] - 128);
            tmp.resize(raw_bytes);
            const size_t half = (raw_bytes + 1) / 2;
            for (size_t i = 0; i < raw_bytes; ++i) tmp[i] = (i & 1) ? z[half + i / 2] : z[i / 2];
            data = tmp.data();
        } else if (size != raw_bytes) {
            refuse("corrupt EXR (chunk size)");
        }
        for (int l = 0; l < lines; ++l) {
            const size_t row = (size_t)(h - 1 - (y0 + l)); // flipped: the file's bottom row is row 0
            const uint8_t* p = data + (size_t)l * line_bytes;
            for (size_t c = 0; c < channels.size(); ++c) {
                const int sz = channels[c].type == 1 ? 2 : 4;
                const int s = slot[c];
                const bool use = s >= 0 && (s < 4 ? (rgb || s == 3) : !rgb);
                if (use)
                    for (int64_t x = 0; x < w; ++x) {
                        float v;
                        if (sz == 2) {
                            v = half_to_float((uint16_t)(p[2 * x] | (p[2 * x + 1] << 8)));
                        } else {
                            const uint32_t u = le32(p + 4 * x);
                            std::memcpy(&v, &u, 4);
                        }
                        float* o = px + 4 * (row * (size_t)w + (size_t)x);
                        if (s == 4) o[0] = o[1] = o[2] = v;
                        else o[s] = v;
                    }
                p += (size_t)w * sz;
            }
        }
    }
    return img;
}

// ---- Radiance RGBE ----------------------------------------------------------------
LoadedImage read_hdr(const uint8_t* d, size_t n) {
    size_t pos = 0;
    auto line = [&]() {
        std::string s;
        for (;;) {
            if (pos >= n) refuse("truncated HDR (header)");
            const char c = (char)d[pos++];
            if (c == '\n') return s;
            if (s.size() > 1024) refuse("corrupt HDR (header line too long)");
            s += c;
        }
    };
    line(); // "#?RADIANCE" / "#?RGBE", checked by the caller
    bool format = false;
    for (;;) {
        const std::string s = line();
        if (s.empty()) break;
        if (s == "FORMAT=32-bit_rle_rgbe") format = true;
        else if (s.compare(0, 7, "FORMAT=") == 0) refuse("HDR format '" + s.substr(7) + "' is not supported");
    }
    if (!format) refuse("corrupt HDR (no FORMAT line)");
    const std::string res = line();
    long hh = 0, ww = 0;
    char tail = 0;
    if (std::sscanf(res.c_str(), "-Y %ld +X %ld%c", &hh, &ww, &tail) != 2) refuse("HDR orientation '" + res + "' is not supported (-Y h +X w is)");
    check_size(ww, hh);
    const size_t w = (size_t)ww, h = (size_t)hh;
    // the file must be able to hold the image before a buffer of its size exists: a run-length
    // encoded scanline takes 4 bytes and, per component, 2 bytes for every 127 pixels at least
    {
        const size_t rle_line = 4 + 4 * 2 * ((w + 126) / 127), flat_line = 4 * w;
        if (h * std::min(rle_line, flat_line) > n - pos) refuse("truncated HDR (file too short for the image)");
    }
    LoadedImage img;
    img.width = (int32_t)w;
    img.height = (int32_t)h;
    img.format = IMAGE_FLOAT4;
    img.pixels.resize(w * h * 16);
    float* px = reinterpret_cast<float*>(img.pixels.data());
    auto convert = [&](const uint8_t* rgbe, float* o) {
        if (rgbe[3]) {
            const float f = std::ldexp(1.0f, (int)rgbe[3] - (128 + 8));
            o[0] = rgbe[0] * f;
            o[1] = rgbe[1] * f;
            o[2] = rgbe[2] * f;
        } else {
            o[0] = o[1] = o[2] = 0.0f;
        }
        o[3] = 1.0f;
    };
    std::vector<uint8_t> scan(w * 4);
    for (size_t y = 0; y < h; ++y) {
        float* row = px + (h - 1 - y) * w * 4;
        const bool rle = w >= 8 && w < 32768 && pos + 4 <= n && d[pos] == 2 && d[pos + 1] == 2 && !(d[pos + 2] & 0x80);
        if (rle) {
            if ((size_t)((d[pos + 2] << 8) | d[pos + 3]) != w) refuse("corrupt HDR (scanline width)");
            pos += 4;
            for (int c = 0; c < 4; ++c) {
                size_t x = 0;
                while (x < w) {
                    if (pos >= n) refuse("truncated HDR (scanline " + std::to_string(y) + ")");
                    size_t count = d[pos++];
                    if (count > 128) {
                        count -= 128;
                        if (pos >= n) refuse("truncated HDR (scanline " + std::to_string(y) + ")");
                        if (x + count > w) refuse("corrupt HDR (run past the scanline)");
                        const uint8_t v = d[pos++];
                        while (count--) scan[4 * x++ + c] = v;
                    } else {
                        if (count == 0 || x + count > w) refuse("corrupt HDR (run past the scanline)");
                        if (pos + count > n) refuse("truncated HDR (scanline " + std::to_string(y) + ")");
                        while (count--) scan[4 * x++ + c] = d[pos++];
                    }
                }
            }
            for (size_t x = 0; x < w; ++x) convert(&scan[4 * x], row + 4 * x);
        } else {
            if (pos + 4 * w > n) refuse("truncated HDR (scanline " + std::to_string(y) + ")");
            for (size_t x = 0; x < w; ++x) convert(d + pos + 4 * x, row + 4 * x);
            pos += 4 * w;
        }
    }
    return img;
}

} // namespace

uint8_t byte_color_to_linear(uint8_t c) {
    const float v = c / 255.0f;
    const float l = v <= 0.04045f ? v / 12.92f : std::pow((v + 0.055f) / 1.055f, 2.4f);
    return (uint8_t)std::min<int>(255, (int)std::floor(l * 255));
}

std::vector<uint8_t> zlib_inflate(const uint8_t* data, size_t n, size_t expected) {
    try {
        return zlib_inflate_or_refuse(data, n, expected);
    } catch (const Reason& r) {
        throw std::runtime_error(r.text);
    }
}

LoadedImage load_image_memory(const uint8_t* d, size_t n, const std::string& name, bool linear) {
    static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    try {
        if (n >= 8 && !std::memcmp(d, png_sig, 8)) return read_png(d, n, linear);
        if (n >= 4 && d[0] == 0x76 && d[1] == 0x2f && d[2] == 0x31 && d[3] == 0x01) return read_exr(d, n);
        if ((n >= 11 && !std::memcmp(d, "#?RADIANCE\n", 11)) || (n >= 7 && !std::memcmp(d, "#?RGBE\n", 7))) return read_hdr(d, n);
        if (n >= 2 && d[0] == 0xff && d[1] == 0xd8) refuse("JPEG is not supported (PNG, OpenEXR and Radiance .hdr are)");
        if (n < 8) refuse("truncated file (" + std::to_string(n) + " bytes)");
        refuse("unknown image format (PNG, OpenEXR and Radiance .hdr are read)");
    } catch (const Reason& r) {
        throw std::runtime_error("image '" + name + "': " + r.text);
    }
}

LoadedImage load_image_file(const std::string& path, bool linear) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("image '" + path + "': cannot open the file");
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return load_image_memory(bytes.data(), bytes.size(), path, linear);
}

} // namespace igx
