// Source descriptor of the general YUV entry of the image kernel (image.hip): one struct, one entry point.
// A new source parameter is a new field here, in walkai_nos_amd/ops/image.py's NosYuvSrc and in the launcher.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

// One plane: p its first byte, [lo, hi) the storage it lives in (no byte outside is read), pitch and
// bstride the bytes between rows and between batch elements (bstride possibly negative).
typedef struct NosYuvPlane {
  const void* p;
  const void* lo;
  const void* hi;
  long long pitch;
  long long bstride;
} NosYuvPlane;

typedef struct NosYuvSrc {
  int size;          // sizeof(NosYuvSrc): checked first, a mismatch is an error
  int layout;        // 0 planar (y, u, v) | 1 semi-planar (y, interleaved chroma pairs) | 2 packed 4:2:2 (one plane)
  int hsub, vsub;    // log2 chroma subsampling: (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4; packed is (1, 0)
  int sample_bytes;  // 1 | 2 (little-endian); packed is 1
  int depth, shift;  // code = (word >> shift) & ((1 << depth) - 1); depth 8 (shift 0) when sample_bytes is 1,
                     // else 10 or 12 with shift 0 (value in the low bits) or 16 - depth (in the high bits)
  int order;         // semi-planar: 0 UV / 1 VU; packed: 0 YUYV / 1 UYVY / 2 YVYU; planar: 0
  NosYuvPlane plane[3];  // planar y, u, v; semi-planar y, pairs; packed the one plane (the rest ignored)
  int tab[12];       // ops/image.py's yuv_table: the matrix times 2^(8 + depth) by rows (R, G, B) x (Y, U, V),
                     // each below 2^23 in size, then the offsets taken from Y, U and V (codes of that depth)
  int chroma;        // 0 nearest: luma (r, c) takes chroma (r >> vsub, c >> hsub) | 1 bilinear (hsub = 1 only): the two
                     // nearest samples per subsampled axis by weights in quarters, (sum + 8) >> 4, clamped at the edges
  int siting;        // bilinear: bit 0 chroma is co-sited with the even luma columns (else centred between a pair),
                     // bit 1 the same for rows: 1 "left" (MPEG-2, H.264), 0 "center" (JPEG), 3 "topleft", 2 "top"
} NosYuvSrc;

// src, then the arguments of nos_image_patch_planes_u8 from `planes` on.
int nos_image_patch_planes_yuv(const NosYuvSrc* src, void* planes, float* pixels, const int* yidx, const float* ywt,
                               const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                               const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh, int gw,
                               int wgs, void* stream);

int nos_image_yuv_max_footprint(void);

// The tables of a PQ or HLG source (ops/image.py's hdr_tables, on the device): the source's R'G'B' codes are not cut
// to 8 bits but taken, at the source's depth, through lut1 (tone-mapped linear light, 16383 = SDR white), the gamut
// matrix in 2^-12 fixed point, clip((sum + 2048) >> 12, 0, 16383), and lut2 (the sRGB byte). The kernel knows no
// transfer function. A descriptor of its own: NosYuvSrc is as it was.
typedef struct NosYuvHdr {
  int size;          // sizeof(NosYuvHdr): checked first, a mismatch is an error
  int entries;       // of lut1: 1 << depth of the source
  const void* lut1;  // uint16 [entries], device memory: values up to 16383
  const void* lut2;  // uint8 [16384], device memory
  int gamut[9];      // by rows (R, G, B out) x (R, G, B in), each below 2^15 in size
} NosYuvHdr;

// nos_image_patch_planes_yuv of such a source: 16-bit samples, planar or semi-planar. Every check of that entry, then
// those of the tables; nothing is launched unless all pass.
int nos_image_patch_planes_yuv_hdr(const NosYuvSrc* src, const NosYuvHdr* hdr, void* planes, float* pixels,
                                   const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab,
                                   int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b, int B,
                                   int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream);

// B tiles of h x w (the common arguments' sizes) of one frame of frame_h x frame_w, which src describes; hdr is null
// for an SDR source. origins: host array [B][2] of (first row, first column); table: the same on the device, int32.
// frames: the batch src's planes hold, which must be 1. As the two entries above on the crops of the converted frame,
// bit for bit; nothing is launched unless their checks pass for the frame and every tile lies inside it.
int nos_image_patch_planes_yuv_tiles(const NosYuvSrc* src, const NosYuvHdr* hdr, const int* origins, const int* table,
                                     int frame_h, int frame_w, int frames, void* planes, float* pixels,
                                     const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab,
                                     int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b, int B,
                                     int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream);

#ifdef __cplusplus
}
#endif
