// The host path of Device::tonemap / Device::imageinfo as the facade ran it
// before the device kernels (a copy of the whole film to the host, then the
// loops of host/film_tools.h), for tools/post_bench.py to time next to the
// device entry points; and glare_host (host/glare_model.h), the host statement of
// the glare kernel.  Built by the script with g++ -O2 into a shared library.
#include "film_tools.h"
#include "glare_model.h"

extern "C" void post_host_tonemap(const float* rgb, size_t pixels, float scale, int method, int use_gamma, float exposure_factor,
                                  float exposure_offset, uint32_t* out) {
    igx::tonemap_film(rgb, pixels, scale, method, use_gamma != 0, exposure_factor, exposure_offset, out);
}

extern "C" float post_host_imageinfo(const float* rgb, size_t w, size_t h, float scale, size_t bins, int* hr, int* hg, int* hb, int* hl) {
    return igx::imageinfo_film(rgb, w, h, scale, bins, hr, hg, hb, hl, true, true).avg;
}

extern "C" void post_host_glare(const float* rgb, int w, int h, const igx_camera* camera, const igx_glare_settings* settings,
                                uint32_t* overlay, igx_glare_output* out) {
    igx::glare_host(rgb, w, h, igxd::make_camera_model(*camera, w, h), *settings, overlay, out);
}
