// Feeds host/image_io.cpp damaged files (tests/test_image_io.py builds this with
// the address and undefined-behaviour sanitizers): every fixture given on the
// command line must load whole, be refused with a message naming it when cut at
// any length, and either load or be refused -- never crash -- with single bytes
// changed at a fixed stride.
#include "image_io.h"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string path = argv[a];
        std::ifstream in(path, std::ios::binary);
        std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (file.empty()) {
            std::printf("%s: cannot read\n", path.c_str());
            return 2;
        }
        igx::LoadedImage whole;
        try {
            whole = igx::load_image_memory(file.data(), file.size(), path, false);
        } catch (const std::exception& e) {
            std::printf("%s: whole file refused: %s\n", path.c_str(), e.what());
            return 3;
        }
        size_t refused = 0, loaded = 0;
        for (size_t len = 0; len < file.size(); ++len) {
            // an exact-size copy, so a read past the cut is a heap overflow the sanitizer sees
            std::vector<uint8_t> cut(file.begin(), file.begin() + len);
            try {
                igx::load_image_memory(cut.data(), cut.size(), path, false);
                std::printf("%s: loaded although cut at %zu of %zu bytes\n", path.c_str(), len, file.size());
                ++failures;
            } catch (const std::runtime_error& e) {
                if (std::string(e.what()).find(path) == std::string::npos) {
                    std::printf("%s: message without the file name: %s\n", path.c_str(), e.what());
                    ++failures;
                }
                ++refused;
            }
        }
        const size_t stride = file.size() > 4096 ? 7 : 1;
        for (size_t at = 0; at < file.size(); at += stride)
            for (uint8_t flip : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xff}) {
                std::vector<uint8_t> bad(file);
                bad[at] ^= flip;
                try {
                    const igx::LoadedImage img = igx::load_image_memory(bad.data(), bad.size(), path, false);
                    if (img.pixels.size() != (size_t)img.width * img.height * igx::image_pixel_bytes(img.format)) ++failures;
                    ++loaded;
                } catch (const std::runtime_error&) {
                    ++refused;
                }
            }
        std::printf("%s: %d x %d, %zu refusals, %zu damaged files still loaded\n", path.c_str(), whole.width, whole.height, refused, loaded);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
