// jpeg.h -- frames to baseline JPEG files (include/opk.h "JPEG FRAMES"; the reference's ImageSaver
// behind --write_images_format jpg and --write_video): the tables, the bound, the checks and the
// plain-C++ encoder on the host (host/jpeg.cpp, no device code), and the device route
// (host/jpeg_dev.cpp, kernels/jpeg.hip) (internal).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../kernels/jpeg_dev.h"

namespace opk {

// the header of a w x h file at `quality`, 8 * Q, the zigzag scan and the four code tables
void make_jpeg_tables(JpegTables& t, int w, int h, int quality);
// opk_jpeg_bound; 0 for n <= 0 or an empty frame
size_t jpeg_bound(int n, int w, int h);
// OPK_ERR_ARG for a width or height outside 1..65535 or a quality outside 1..100
void check_jpeg(int w, int h, int quality);
// OPK_ERR_ARG when [dst, dst + capacity) meets [src, src + src_bytes)
void check_jpeg_apart(const uint8_t* dst, size_t capacity, const uint8_t* src, size_t src_bytes);
// opk_jpeg_encode_host after its checks: step and frame_bytes resolved, n > 0
void jpeg_encode_host(uint8_t* dst, size_t capacity, uint64_t* offsets, const uint8_t* bgr,
                      size_t step, size_t frame_bytes, int n, int w, int h, int quality);

}  // namespace opk
