// Image files of image textures (host side, no HIP, no link dependency):
// PNG, scanline OpenEXR and Radiance .hdr, decoded with the semantics of the
// reference's Image.cpp.
//
//  * 8-bit files (PNG) are "packed" (Image::isPacked, Image.cpp:335-341): rows
//    flipped so the file's bottom row is row 0, every colour byte through
//    byte_color_to_linear (Image.cpp:39-41) unless the texture says `linear`,
//    alpha kept; stored RGBA8 (R in the low byte), or MONO8 for 1-channel
//    files.  16-bit PNGs are reduced to their high byte, as stb does.
//  * EXR and HDR load as float RGBA, rows flipped (Image.cpp:559-560); a missing
//    alpha is 1, a single Y channel fills R, G and B.
//
// A tRNS colour key on a grey or RGB PNG is dropped (stb would turn it into an
// alpha channel; nothing reads a texture's alpha): such a file stays MONO8 or
// opaque RGBA8.
// Read: PNG 1/2/4/8/16 bit grey, grey+alpha, RGB, RGBA and palette (with tRNS),
// non-interlaced, all five filters, chunk CRCs and the zlib checksum verified;
// EXR single-part scanline files with compression NONE / ZIPS / ZIP and half or
// float channels in any order; Radiance RGBE, run-length encoded and flat.
// Everything else (JPEG, interlaced PNG, tiled / multipart / otherwise
// compressed EXR, truncated or corrupt data, a side above MAX_IMAGE_SIDE) is
// refused with a std::runtime_error naming the file and the reason.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace igx {

// values of igx_image::format (include/igx_scene.h)
enum : int32_t { IMAGE_RGBA8 = 0, IMAGE_MONO8 = 1, IMAGE_FLOAT4 = 2 };
constexpr int MAX_IMAGE_SIDE = 16384;

struct LoadedImage {
    int32_t width = 0, height = 0;
    int32_t format = IMAGE_RGBA8;
    std::vector<uint8_t> pixels; // width * height * (4 | 1 | 16) bytes, row 0 = the file's bottom row
};

inline size_t image_pixel_bytes(int32_t format) { return format == IMAGE_FLOAT4 ? 16 : format == IMAGE_MONO8 ? 1 : 4; }

// floor(srgb_invgamma(c / 255) * 255), Image.cpp:31-41
uint8_t byte_color_to_linear(uint8_t c);

// RFC 1950 / 1951: a zlib stream of stored, fixed and dynamic Huffman blocks,
// inflated to exactly `expected` bytes (anything else throws)
std::vector<uint8_t> zlib_inflate(const uint8_t* data, size_t n, size_t expected);

// The format follows the file's first bytes; `name` only labels messages.
LoadedImage load_image_memory(const uint8_t* data, size_t n, const std::string& name, bool linear);
LoadedImage load_image_file(const std::string& path, bool linear);

} // namespace igx
