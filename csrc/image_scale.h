// The scaler of the image library (image.hip): a frame resized into a second surface of the same layout, depth,
// subsampling and byte order, plane by plane, by the exact area average the chips define per axis. The first image
// kernel whose output is a frame.
//  * rescale_k<WIDE> — one launch; the rule is exact integers, ops/image.py's rescale states it in full.
//
// Storage planes, periods and slots. A surface is one to three *storage planes* (packed pixels: one; planar: three;
// semi-planar: Y and the pairs; packed 4:2:2: one). A row of a storage plane is a run of *slots* of one sample (a byte
// or a 16-bit word) that repeats with a *period* of P slots: P = 1 (a planar plane), 2 (a UV pair), 3 (RGB), 4 (RGBA:
// the fourth slot belongs to no component; YUY2: a macropixel). Every slot of a period belongs to a *class* of
// components that share a lattice — class 0 with (pw, PW) source and target columns, and in a macropixel class 1, the
// chroma, with half of them — and a class has 1 << ns columns in a period (2 for a macropixel's luma). Source and
// target agree in kind, so one table of P slots (ScalePlane::slots) describes both sides.
//
// How the work is split. The grid is a flat list of tiles of the *target*: for every storage plane, (column tiles of
// SCALE_T / P whole periods) x (bands of `band` rows). It depends on the two sizes alone. A workgroup of SCALE_T = 256
// threads owns whole periods, so both components of a UV pair, the four bytes of a macropixel (samples of three
// components on two lattices) and the colour bytes of a pixel are written by one workgroup, and no two workgroups
// write the same word. Thread tid owns *entry* tid of the tile: slot tid % P of period tid / P, in every row of the
// band. band is SCALE_BAND = 8 rows, halved by the host while the grid would hold fewer than 1024 workgroups (so a
// thumbnail still spreads over the CUs).
//
// How data moves. The band's rows J0 .. J1 - 1 cover source rows floor(J0 ph / PH) .. ceil(J1 ph / PH) - 1, the tile's
// columns a range of source periods (the union over the classes). The footprint is streamed through LDS in chunks of
// SCALE_ROWS = 8 rows x at most SCALE_SLOTS = 1024 slots (whole periods). Staging walks every row in aligned dwords
// (the row's first byte rounded down to a multiple of 4; a dword that straddles the chunk's first or last byte is
// read byte by byte, so no byte outside the chunk is read) and extracts the codes on the way in — (word >> shift) &
// mask — to 16-bit LDS entries at the slot's own index: an interleaved pair and a macropixel need no reordering, the
// horizontal pass computes the slot it wants. Horizontal pass: for each staged row the thread sums, over the source
// columns its output column overlaps, overlap x code: below pw * maxcode < 2^25, a 32-bit register. Vertical pass,
// fused: that sum goes straight into the thread's `band` accumulators, each times the row's overlap with the output
// row (a wave-uniform integer), so the horizontal sums never touch LDS and a column chunk just adds its part. The
// weights are lattice arithmetic in both passes (min / max of multiples of the four sizes); there are no tables.
//
// Width of the sums. A full sum is below A * maxcode, A = ph * pw. The host takes rescale_k<false> — 32-bit
// accumulators and one 32-bit division — where A * (maxcode + 1) <= 2^32 in every class (8 bits: up to 2^24 source
// samples, 10 bits: 2^22), and else rescale_k<true>: 64-bit accumulators (v_mad_u64_u32), and per output one
// multiplication by the host's 1.0 / A in fp64 with a correction step: the quotient is below 4096 and the product's
// relative error below 2^-50, so the estimate is off by at most one and `r = s - q A` puts it right. Exact for every
// size inside the limits.
//
// Stores. One per storage unit where the layout allows: a UV pair as one 16- or 32-bit word by its even lane (the odd
// lane's code comes by a cross-lane shuffle), a full macropixel as one dword by its first lane (three shuffles), a
// 16-bit sample as one word; a pair or a macropixel whose address is not a multiple of its size, the half-filled last
// macropixel of an odd width, 8-bit planar samples and packed pixels are stored sample by sample (a three-byte pixel
// has no word; the fourth byte of RGBA is never written). Consecutive lanes store consecutive addresses.
//
// LDS: SCALE_ROWS x SCALE_ROWH halfwords = 16.2 KB a workgroup, static; nine workgroups a CU by LDS. A staged row is
// SCALE_ROWH = 1034 halfwords = 517 dwords (odd), so the rows of a chunk start in different banks. Horizontal pass:
// lanes are consecutive entries; enlarging, neighbours read the same halfword (a broadcast); shrinking by f they read
// halfwords f P apart in a loop whose length differs by at most one between lanes. Registers: the compiler reports
// no scratch; the accumulators are 8 (narrow) or 16 (wide) VGPRs.
//
// Matrix instructions are left out: the weights differ per output column and the sums must be exact integers of up to
// 38 bits. What binds the kernel was not measured: it runs 4 to 26 times above a copy of the source's bytes, so not
// at the memory's speed; the LDS reads of the horizontal pass and the vertical pass's SCALE_BAND weights per staged
// row and thread are the supposed costs.
//
// Not measured against their alternatives: SCALE_ROWS = 8 against 4 or 16, the chunk of 1024 slots, the band rule
// (8 rows, halved below 1024 workgroups), testing every row of the band per staged row against the one or two it
// overlaps, a thread per entry against a thread per storage unit, the shuffled word
// stores against stores of single samples, the fp64 reciprocal against a 64-bit division, and dword staging against
// wider loads.
// Included by image.hip alone, after image_overlay.h (PlaneArg).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_stage.h"

namespace {
// threads of a workgroup = entries of a tile; source rows and slots of a chunk; halfwords of a staged row; output rows
// of a band at most; the largest side
constexpr int SCALE_T = 256, SCALE_ROWS = 8, SCALE_SLOTS = 1024, SCALE_ROWH = SCALE_SLOTS + 10, SCALE_BAND = 8;
constexpr int SCALE_MAX_SIDE = 8192;
static_assert((SCALE_ROWH / 2) % 2 == 1 && SCALE_ROWH % 2 == 0, "an odd number of whole dwords a row");
static_assert(SCALE_ROWH >= SCALE_SLOTS + 3 + 3, "a lead of up to three slots, and the last dword's tail");
static_assert(SCALE_MAX_SIDE * SCALE_MAX_SIDE <= 1 << 26 && (SCALE_MAX_SIDE * 4095LL) < (1 << 25),
              "lattice coordinates fit int32, a horizontal sum 25 bits");

// One storage plane of both surfaces. slots: a byte per slot k of a period, (class + 1) | kb << 2 | idx << 4 — class
// -1: no component; idx: which of its class's columns of the period the slot is; kb: the slot of the class's first
// column, so that column x of the class lies at slot (x >> ns) * P + kb + 2 * (x & ((1 << ns) - 1)) of a row.
struct ScalePlane {
  const uint8_t* src;
  uint8_t* dst;
  long long spitch, dpitch;
  double inv[2];     // 1.0 / area
  uint32_t area[2];  // ph * pw by class
  int pw[2], PW[2], ns[2];
  int ph, PH, P;
  uint32_t slots;
  int src_slots;             // slots of a source row
  int tiles_x, bands, first; // column tiles, bands, and the plane's first workgroup in the grid
  int unit;                  // what a store holds: 0 a sample, 1 a pair, 2 a macropixel
};

struct ScaleArgs {
  ScalePlane pl[3];  // (an unused plane's `first` is the grid's size)
  int sb, shift, mask, band;
};

// (sum + A / 2) / A, exactly
template <bool WIDE>
__device__ __forceinline__ uint32_t scale_div(typename std::conditional<WIDE, uint64_t, uint32_t>::type sum, uint32_t A,
                                              double inv) {
  if constexpr (!WIDE) {
    return (sum + A / 2) / A;
  } else {
    const uint64_t s = sum + A / 2;
    uint32_t q = uint32_t(double(s) * inv);
    const int64_t r = int64_t(s) - int64_t(uint64_t(q) * A);
    if (r < 0) --q;
    else if (r >= int64_t(A)) ++q;
    return q;
  }
}

// The trip counts of the loops that hold barriers (the row chunks, the column chunks) come from the kernel's
// arguments and the workgroup's index alone.
template <bool WIDE>
__global__ __launch_bounds__(SCALE_T) void rescale_k(ScaleArgs a) {
  using Acc = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  __shared__ uint16_t s_code[SCALE_ROWS * SCALE_ROWH];
  const int tid = threadIdx.x, wg = blockIdx.x;
  const ScalePlane& p = wg >= a.pl[2].first ? a.pl[2] : wg >= a.pl[1].first ? a.pl[1] : a.pl[0];
  const int sb = a.sb, P = p.P, TP = SCALE_T / P;
  const int tx = (wg - p.first) % p.tiles_x, J0 = (wg - p.first) / p.tiles_x * a.band, J1 = min(J0 + a.band, p.PH);
  const int ph = p.ph, PH = p.PH;

  // the thread's entry: slot k of period `period` of the target row, column I of class c
  const int per = tid / P, k = tid - per * P, period = tx * TP + per;
  const uint32_t info = (p.slots >> (8 * k)) & 255u;
  const int c = int(info & 3u) - 1, kb = int(info >> 2) & 3, idx = int(info >> 4) & 1, c1 = c > 0;
  const int pw = c1 ? p.pw[1] : p.pw[0], PW = c1 ? p.PW[1] : p.PW[0], ns = c1 ? p.ns[1] : p.ns[0];
  const int I = (period << ns) + idx;
  const bool active = per < TP && c >= 0 && I < PW;
  // on the lattice of pw * PW units the output column is [vlo, vhi), source column x is [x PW, (x + 1) PW)
  const int vlo = active ? I * pw : 0, vhi = active ? vlo + pw : 0;
  const int xs = active ? vlo / PW : 0, xe = active ? (vhi + PW - 1) / PW : 0;

  // the source periods under the tile: the union over the classes
  int plo = 1 << 30, phi = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (p.PW[q] == 0) continue;
    const int I0 = (tx * TP) << p.ns[q], I1 = min(((tx + 1) * TP) << p.ns[q], p.PW[q]);
    if (I0 >= I1) continue;
    const int xlo = I0 * p.pw[q] / p.PW[q], xhi = (I1 * p.pw[q] + p.PW[q] - 1) / p.PW[q];
    plo = min(plo, xlo >> p.ns[q]), phi = max(phi, ((xhi - 1) >> p.ns[q]) + 1);
  }
  const int T0 = J0 * ph / PH, T1 = (J1 * ph + PH - 1) / PH;  // the band's source rows
  const int CPER = SCALE_SLOTS / P;                           // periods of a column chunk

  Acc acc[SCALE_BAND];
#pragma unroll
  for (int i = 0; i < SCALE_BAND; ++i) acc[i] = 0;

  for (int t0 = T0; t0 < T1; t0 += SCALE_ROWS) {
    const int nr = min(SCALE_ROWS, T1 - t0);
    for (int pc = plo; pc < phi; pc += CPER) {
      const int np = min(CPER, phi - pc), slot0 = pc * P;
      const int nbytes = (min((pc + np) * P, p.src_slots) - slot0) * sb;
      const uint8_t* const first = p.src + (long long)t0 * p.spitch + (long long)slot0 * sb;
      __syncthreads();  // the last chunk's reads lie before this barrier
      const int ndw = (nbytes + 6) >> 2;
      for (int e = tid; e < nr * ndw; e += SCALE_T) {
        const int r = e / ndw, d = e - r * ndw;
        const uint8_t* const row = first + r * p.spitch;
        const int lb = int(reinterpret_cast<uintptr_t>(row) & 3), b = 4 * d - lb;  // the dword's first byte of the chunk
        if (b >= nbytes) continue;
        uint32_t v = 0;
        if (b >= 0 && b + 4 <= nbytes) {
          v = *reinterpret_cast<const uint32_t*>(row + b);
        } else {
          for (int i = max(-b, 0); i < min(4, nbytes - b); ++i) v |= uint32_t(row[b + i]) << (8 * i);
        }
        if (sb == 2) {
          const uint32_t lo = ((v & 0xffffu) >> a.shift) & a.mask, hi = ((v >> 16) >> a.shift) & a.mask;
          *reinterpret_cast<uint32_t*>(s_code + r * SCALE_ROWH + 2 * d) = lo | hi << 16;
        } else {
          uint32_t* q = reinterpret_cast<uint32_t*>(s_code + r * SCALE_ROWH + 4 * d);
          q[0] = (v & 255u) | (v >> 8 & 255u) << 16, q[1] = (v >> 16 & 255u) | (v >> 24) << 16;
        }
      }
      __syncthreads();
      // the chunk's columns of the thread's class
      const int xa = max(xs, pc << ns), xb = min(xe, (pc + np) << ns);
      if (xa >= xb) continue;
      for (int r = 0; r < nr; ++r) {
        const int lead = int(reinterpret_cast<uintptr_t>(first + r * p.spitch) & 3) / sb;
        const uint16_t* const row = s_code + r * SCALE_ROWH + lead - slot0 + kb;
        uint32_t sum = 0;
        for (int x = xa, lo = xa * PW; x < xb; ++x, lo += PW)
          sum += uint32_t(min(lo + PW, vhi) - max(lo, vlo)) * row[(x >> ns) * P + 2 * (x & ns)];
        const int tlo = (t0 + r) * PH;
#pragma unroll
        for (int i = 0; i < SCALE_BAND; ++i) {
          const int ulo = (J0 + i) * ph, wgt = min(tlo + PH, ulo + ph) - max(tlo, ulo);
          if (J0 + i < J1 && wgt > 0) acc[i] += Acc(uint32_t(wgt)) * sum;
        }
      }
    }
  }

  const uint32_t A = c1 ? p.area[1] : p.area[0];
  const double inv = c1 ? p.inv[1] : p.inv[0];
  const int unit = p.unit;
#pragma unroll
  for (int i = 0; i < SCALE_BAND; ++i) {
    if (J0 + i >= J1) break;
    const uint32_t v = active ? scale_div<WIDE>(acc[i], A, inv) << a.shift : 0u;
    uint8_t* const at = p.dst + (J0 + i) * p.dpitch + ((long long)period * P + k) * sb;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(at);
    bool single = active;  // the thread stores its own sample
    if (unit == 1) {
      // a pair: both lanes are active or neither is
      const uint32_t other = __shfl_xor(v, 1);
      if (active && ((addr - k * sb) & (2 * sb - 1)) == 0) {
        single = false;
        if (k == 0 && sb == 1) *reinterpret_cast<uint16_t*>(at) = uint16_t(v | other << 8);
        if (k == 0 && sb == 2) *reinterpret_cast<uint32_t*>(at) = v | other << 16;
      }
    } else if (unit == 2) {
      // a macropixel: its bytes, and which of them are samples of the frame
      uint32_t w = active ? v << (8 * k) : 0u, m = active ? 1u << k : 0u;
      w |= __shfl_xor(w, 1), m |= __shfl_xor(m, 1);
      w |= __shfl_xor(w, 2), m |= __shfl_xor(m, 2);
      if (m == 15u && ((addr - k) & 3) == 0) {
        single = false;
        if (k == 0) *reinterpret_cast<uint32_t*>(at) = w;
      }
    }
    if (single) {
      if (sb == 2) *reinterpret_cast<uint16_t*>(at) = uint16_t(v);
      else *at = uint8_t(v);
    }
  }
}
}  // namespace
