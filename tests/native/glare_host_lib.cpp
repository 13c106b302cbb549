// glare_host of host/glare_model.h behind a C entry point, so that
// tests/test_glare_gpu.py can call the host restatement of k_glare_scan (same
// arithmetic, same order of additions) through ctypes.  Compiled by the test
// with g++ -ffp-contract=off as a shared library; no libigx, no GPU.
#include "glare_model.h"

extern "C" void glare_host_c(const float* film, int w, int h, const igx_camera* camera, const igx_glare_settings* settings,
                             uint32_t* overlay, igx_glare_output* out) {
    igx::glare_host(film, w, h, igxd::make_camera_model(*camera, w, h), *settings, overlay, out);
}
