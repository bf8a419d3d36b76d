// Host replay of the device JPEG decoder: every stage of x3d-tf_amd/csrc/jpeg.hip is __host__ __device__, so this
// stand-alone program includes the file and runs the stages serially on the CPU, in the order and under the conditions
// of x3d_jpeg_decode's three launches:
//   x3d_jpeg_parse -> huff_limits x 8 -> huff_look x 4096 -> entropy_decode -> idct_block over every block ->
//   color_pixel over every pixel (the last two only when the status is X3D_JPEG_OK).
// Every buffer is a heap allocation of exactly the size the device path gets (the input bytes, the scratch at
// scratch_bytes, the output at H * W * 3), so a sanitizer build (-fsanitize=address,undefined) sees any access past them.
//
//   jpeg_replay LIST      LIST: one "<input.jpg> <output.bin>" pair per line
// <output.bin>: int32 status, int32 height, int32 width, then height * width * 3 RGB bytes when the status is 0.
// status: X3D_JPEG_* as the device reports it, or -1 for a frame larger than kMaxPixels (a damaged header can claim
// 65535 x 65535), which the replay does not allocate.  tests/test_jpeg_replay.py builds and drives it.
#include "../x3d-tf_amd/csrc/jpeg.hip"

#include <stdarg.h>

#include <string>
#include <vector>

// the two symbols csrc/common.h expects from api.cpp
void x3d_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
thread_local X3dDescribe x3d_describe = {nullptr, 0};

namespace {

constexpr long long kMaxPixels = 1ll << 22;

bool read_file(const char* path, unsigned char** data, int* len) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* p = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);   // exactly the file (malloc(0) may return NULL)
  const bool ok = p && fread(p, 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  if (!ok) { free(p); return false; }
  *data = p;
  *len = (int)n;
  return true;
}

// one image through the decoder; *rgb (malloc, height * width * 3) is set when the returned status is X3D_JPEG_OK
int replay(const unsigned char* data, int len, int* height, int* width, unsigned char** rgb) {
  x3d_jpeg_image d;
  memset(&d, 0, sizeof(d));
  long long scratch_bytes = 0;
  const unsigned char* ptrs[1] = {data};
  const int lens[1] = {len};
  if (x3d_jpeg_parse(ptrs, lens, 1, &d, &scratch_bytes) != X3D_OK) return X3D_JPEG_MALFORMED;
  *height = d.height;
  *width = d.width;
  if (d.status != X3D_JPEG_OK) return d.status;
  const long long px = (long long)d.height * d.width;
  if (px > kMaxPixels) return -1;
  d.data_off = 0;
  d.data_len = len;
  unsigned char* out = (unsigned char*)malloc((size_t)px * 3);
  unsigned char* scratch = (unsigned char*)malloc((size_t)scratch_bytes);
  HuffLds* t = (HuffLds*)malloc(sizeof(HuffLds));
  if (!out || !scratch || !t) { fprintf(stderr, "out of memory\n"); exit(2); }
  d.out = out;
  const long long nb = blocks_of(&d);
  memset(scratch, 0, (size_t)(d.coef_off + nb * 128));                // x3d_jpeg_decode's hipMemsetAsync
  memset(scratch + d.plane_off, 0xA5, (size_t)(scratch_bytes - d.plane_off));
  memset(out, 0x5A, (size_t)px * 3);
  // launch 1: the wave builds the tables, lane 0 decodes the scan
  for (int tb = 0; tb < kTables; tb++) huff_limits(data, d, *t, tb);
  for (int e = 0; e < kTables << kLook; e++) huff_look(*t, e);
  int status = entropy_decode(data, d, *t, (short*)scratch + d.coef_off / 2);
  if (status == X3D_JPEG_OK)                                          // launch 2: a block out of range reports the image
    for (long long b = 0; b < nb; b++)
      if (!idct_block(d, scratch, b)) status = X3D_JPEG_CORRUPT;
  if (status == X3D_JPEG_OK) {
    for (long long i = 0; i < px; i++) color_pixel(d, scratch, i);    // launch 3
    *rgb = out;
  } else {
    free(out);
  }
  free(t);
  free(scratch);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s LIST   (lines: <input.jpg> <output.bin>)\n", argv[0]);
    return 2;
  }
  FILE* lf = fopen(argv[1], "r");
  if (!lf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<std::pair<std::string, std::string>> jobs;
  char a[4096], b[4096];
  while (fscanf(lf, "%4095s %4095s", a, b) == 2) jobs.emplace_back(a, b);
  fclose(lf);
  for (const auto& job : jobs) {
    unsigned char* data = nullptr;
    int len = 0;
    if (!read_file(job.first.c_str(), &data, &len)) { fprintf(stderr, "cannot read %s\n", job.first.c_str()); return 2; }
    int hw[2] = {0, 0};
    unsigned char* rgb = nullptr;
    const int status = replay(data, len, &hw[0], &hw[1], &rgb);
    free(data);
    FILE* of = fopen(job.second.c_str(), "wb");
    if (!of) { fprintf(stderr, "cannot write %s\n", job.second.c_str()); return 2; }
    const int head[3] = {status, hw[0], hw[1]};
    fwrite(head, sizeof(int), 3, of);
    if (status == X3D_JPEG_OK) fwrite(rgb, 1, (size_t)hw[0] * hw[1] * 3, of);
    free(rgb);
    if (fclose(of) != 0) { fprintf(stderr, "cannot write %s\n", job.second.c_str()); return 2; }
  }
  return 0;
}
