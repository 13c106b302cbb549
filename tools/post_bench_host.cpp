// The host path of Device::tonemap / Device::imageinfo as the facade ran it
// before the device kernels (a copy of the whole film to the host, then the
// loops of host/film_tools.h), for tools/post_bench.py to time next to the
// device entry points.  Built by the script with g++ -O2 into a shared library.
#include "film_tools.h"

extern "C" void post_host_tonemap(const float* rgb, size_t pixels, float scale, int method, int use_gamma, float exposure_factor,
                                  float exposure_offset, uint32_t* out) {
    igx::tonemap_film(rgb, pixels, scale, method, use_gamma != 0, exposure_factor, exposure_offset, out);
}

extern "C" float post_host_imageinfo(const float* rgb, size_t w, size_t h, float scale, size_t bins, int* hr, int* hg, int* hb, int* hl) {
    return igx::imageinfo_film(rgb, w, h, scale, bins, hr, hg, hb, hl, true, true).avg;
}
