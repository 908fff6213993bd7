// Front end of detection and negative mining on gfx950: scale pyramid (bit-exact fixed-point bilinear, k_resize), integral
// images (sum + wrap-around sqsum, k_integral_carry / k_integral_band) and the tilted integral (k_diag_sums, k_tilted_cols)
// of every level of a batch of frames. front_layout lays the levels out, FrontTables::upload puts the tables on the device
// and launch_front queues the kernels (cc_detect_internal.h). Also the building-block entry points cc_resize_linear_exact_u8
// and cc_integral_u8, which run the same kernels on one image.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cc_detect_internal.h"
#include "cc_resize_arith.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// K1: pyramid. One thread = 4 horizontally adjacent output pixels x RESIZE_ROWS consecutive output rows of one scale.
// INTER_LINEAR_EXACT: horizontal 8.8 taps exact in 16 bits, vertical exact in 32 bits, (v + 2^15) >> 16.
// The column taps are looked up once per thread; walking down the rows, the horizontally interpolated values of a source
// row are reused when the next output row starts on it (the usual case below scale 2), so an output pixel costs about
// one new source row (2 byte loads) instead of two rows and two table lookups.
// ------------------------------------------------------------------------------------------------
// A block is 4 wavefronts = 4 consecutive bands of RESIZE_ROWS output rows x 64 words (256 columns): a wavefront stays
// inside one band, so its row taps are wave-uniform (scalar loads).
constexpr int RESIZE_ROWS = 8;
struct __attribute__((packed, aligned(1))) Bytes16 {  // 16 bytes at any address (the hardware takes unaligned global loads)
  unsigned d[4];
};
__host__ __device__ inline int resize_blocks(int pitch8, int h) {
  return ((pitch8 / 4 + 63) / 64) * (((h + RESIZE_ROWS - 1) / RESIZE_ROWS + 3) / 4);
}
// Appends one scale's column taps, padded with copies of the last tap to a multiple of 4 entries (so does every earlier
// scale: the returned offset is a multiple of 4): a thread fetches the taps of its 4 columns with one 16-byte and one
// 8-byte load, and the columns of the row padding get the last column's taps (their output is masked anyway).
static int append_column_taps(const AxisTaps& t, std::vector<int>& ofs, std::vector<uint16_t>& w1) {
  const int at = (int)ofs.size();
  ofs.insert(ofs.end(), t.ofs.begin(), t.ofs.end());
  w1.insert(w1.end(), t.w1.begin(), t.w1.end());
  while (ofs.size() % 4) {
    ofs.push_back(t.ofs.back());
    w1.push_back(t.w1.back());
  }
  return at;
}

__global__ __launch_bounds__(256) void k_resize(const uint8_t* __restrict__ frames, size_t row_stride, size_t frame_stride,
                                                int src_w, int src_h, uint8_t* __restrict__ pyr, size_t pyr_frame_bytes,
                                                const ScaleDev* __restrict__ sd, int nscales,
                                                const int* __restrict__ blk_first, const int* __restrict__ xofs,
                                                const uint16_t* __restrict__ xw1, const int* __restrict__ yofs,
                                                const uint16_t* __restrict__ yw1, int32_t* __restrict__ hbuf, size_t h_frame_elems,
                                                int nchan, int sq) {
  const int s = find_segment(blk_first, nscales, blockIdx.x);
  const ScaleDev S = sd[s];
  const int wpr = S.pitch8 >> 2, nxb = (wpr + 63) >> 6;
  const int bi = blockIdx.x - blk_first[s];
  const int bb = bi / nxb, xb = bi - bb * nxb;
  const int band = bb * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xw = xb * 64 + (threadIdx.x & 63);
  const int ya = band * RESIZE_ROWS;
  if (ya >= S.h || xw >= wpr) return;
  const uint8_t* src = frames + (size_t)blockIdx.y * frame_stride;
  int x0[4], x1[4];
  unsigned wx0[4], wx1[4];
  {  // taps of columns 4 xw .. 4 xw + 3 (the tables are padded to the row pitch, see append_column_taps)
    const int4 o = *reinterpret_cast<const int4*>(xofs + S.xtab_ofs + xw * 4);
    const uint2 w = *reinterpret_cast<const uint2*>(xw1 + S.xtab_ofs + xw * 4);
    x0[0] = o.x, x0[1] = o.y, x0[2] = o.z, x0[3] = o.w;
    wx1[0] = w.x & 0xFFFFu, wx1[1] = w.x >> 16, wx1[2] = w.y & 0xFFFFu, wx1[3] = w.y >> 16;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      wx0[k] = 256u - wx1[k];
      x1[k] = min(x0[k] + 1, src_w - 1);
    }
  }
  // Up to scale ~4.6 the 8 source bytes a row contributes to the thread's 4 columns lie within 16 bytes: they come in
  // with ONE (unaligned) 16-byte load from `start` and are picked out with byte permutes whose selectors are fixed per
  // thread -- instead of 8 single-byte loads per source row, which is what the kernel's time went into.
  const int start = min(x0[0], src_w - 16);  // x0 / x1 do not decrease with k: x0[0] is the first, x1[3] the last byte
  const bool wide = src_w >= 16 && x1[3] - start <= 15;
  unsigned sel0 = 0, sel1 = 0, low0 = 0, low1 = 0;  // per tap: byte index within its 8-byte half, 0xFF where it is the low half
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int o0 = x0[k] - start, o1 = x1[k] - start;
    sel0 |= (unsigned)(o0 & 7) << (8 * k);
    sel1 |= (unsigned)(o1 & 7) << (8 * k);
    low0 |= (o0 < 8 ? 0xFFu : 0u) << (8 * k);
    low1 |= (o1 < 8 ? 0xFFu : 0u) << (8 * k);
  }
  auto hrow = [&](int yy, unsigned* h) {  // horizontal interpolation of source row yy at the 4 columns
    const uint8_t* r = src + (size_t)yy * row_stride;
    if (wide) {
      const Bytes16 v = *reinterpret_cast<const Bytes16*>(r + start);
      // __builtin_amdgcn_perm(hi, lo, sel): byte j of the result = byte sel[j] (0..7) of the 8 bytes {lo, hi}
      const unsigned a_lo = __builtin_amdgcn_perm(v.d[1], v.d[0], sel0), a_hi = __builtin_amdgcn_perm(v.d[3], v.d[2], sel0);
      const unsigned b_lo = __builtin_amdgcn_perm(v.d[1], v.d[0], sel1), b_hi = __builtin_amdgcn_perm(v.d[3], v.d[2], sel1);
      const unsigned t0 = (a_lo & low0) | (a_hi & ~low0), t1 = (b_lo & low1) | (b_hi & ~low1);
#pragma unroll
      for (int k = 0; k < 4; k++) h[k] = resize_lerp_h(wx0[k], wx1[k], (t0 >> (8 * k)) & 255u, (t1 >> (8 * k)) & 255u);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) h[k] = resize_lerp_h(wx0[k], wx1[k], r[x0[k]], r[x1[k]]);
    }
  };
  unsigned hc[4] = {0, 0, 0, 0};
  int cached = -1;  // source row whose interpolation hc holds
  unsigned cs[4] = {0, 0, 0, 0}, cq[4] = {0, 0, 0, 0};  // the band's column sums of the pixels and of their squares
  uint8_t* dst = pyr + (size_t)blockIdx.y * pyr_frame_bytes + S.img_ofs;
  const int yb = min(ya + RESIZE_ROWS, S.h);
  for (int y = ya; y < yb; y++) {
    const int y0 = yofs[S.ytab_ofs + y];
    const unsigned wy1 = yw1[S.ytab_ofs + y], wy0 = 256u - wy1;
    const int y1 = min(y0 + 1, src_h - 1);
    unsigned h0[4], h1[4];
    if (y0 == cached) {
#pragma unroll
      for (int k = 0; k < 4; k++) h0[k] = hc[k];
    } else
      hrow(y0, h0);
    if (y1 == y0) {
#pragma unroll
      for (int k = 0; k < 4; k++) h1[k] = h0[k];
    } else
      hrow(y1, h1);
    unsigned packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned v = (xw * 4 + k < S.w) ? resize_lerp_v(wy0, wy1, h0[k], h1[k]) : 0u;
      packed |= v << (8 * k);
      cs[k] += v;
      cq[k] += v * v;
      hc[k] = h1[k];
    }
    cached = y1;
    reinterpret_cast<unsigned*>(dst + (size_t)y * S.pitch8)[xw] = packed;
  }
  if (!hbuf) return;
  // Band totals for the integral kernels (K2): a resize band is an integral band, so this thread holds all of H[band]'s
  // pixels of its 4 columns. The padding columns up to pitchI are written as 0: the quad behind the last pixel word exists
  // in pitchI but not in pitch8 when w is a multiple of 4 and has no thread of its own.
  const size_t hofs = S.h_ofs + (size_t)band * S.pitchI + (size_t)xw * 4;
  const bool pad_quad = xw == wpr - 1 && S.pitchI > S.pitch8;
  int32_t* hs = hbuf + ((size_t)blockIdx.y * nchan + 0) * h_frame_elems + hofs;
  *reinterpret_cast<int4*>(hs) = make_int4((int)cs[0], (int)cs[1], (int)cs[2], (int)cs[3]);
  if (pad_quad) *reinterpret_cast<int4*>(hs + 4) = make_int4(0, 0, 0, 0);
  if (sq) {
    int32_t* hq = hbuf + ((size_t)blockIdx.y * nchan + 1) * h_frame_elems + hofs;
    *reinterpret_cast<int4*>(hq) = make_int4((int)cq[0], (int)cq[1], (int)cq[2], (int)cq[3]);
    if (pad_quad) *reinterpret_cast<int4*>(hq + 4) = make_int4(0, 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------
// K2: integral images in one pass over the pixels (plus a tiny carry pass). The image is cut into bands of INT_BAND rows;
// H[b][x] = the sum of band b's rows at pixel column x (its column sums), per channel:
//   k_resize / k_band_colsums : write H[b][x] -- the pyramid kernel has a band's pixels in registers (RESIZE_ROWS ==
//                               INT_BAND); callers that bring their own level (cc_integral_u8) run k_band_colsums on it;
//   k_integral_carry          : H[b][x] <- sum of H over the bands above b (exclusive scan down the bands, in place);
//   k_integral_band           : one wavefront owns one band of one scale and walks it left to right in chunks of 256 columns
//                               (64 lanes x 4 px): per row an in-register prefix of the lane's 4 px, a DPP wave scan of the
//                               lane totals and a carry into the next chunk; rows accumulate downwards in registers,
//                               starting from the same prefix of H[b] (the rows above the band: prefix along x and sum down
//                               the bands commute), and every row is written as the finished integral.
// sum and sqsum use u32 wrap-around arithmetic throughout (the detector's CV_32S squared sums).
// ------------------------------------------------------------------------------------------------
constexpr int INT_BAND = 8;
static_assert(RESIZE_ROWS == INT_BAND, "k_resize writes the column sums of the integral kernels' bands");

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
// inclusive prefix sum over the 64 lanes (row_shr 1/2/4/8 inside rows of 16, then row_bcast 15 / 31 across rows)
__device__ __forceinline__ unsigned wave_scan_u32(unsigned v) {
  v += dpp_u32<0x111, 0xF>(v);
  v += dpp_u32<0x112, 0xF>(v);
  v += dpp_u32<0x114, 0xF>(v);
  v += dpp_u32<0x118, 0xF>(v);
  v += dpp_u32<0x142, 0xA>(v);
  v += dpp_u32<0x143, 0xC>(v);
  return v;
}
// One row of a chunk: p = the lane's 4 entries, carry = the row's total over the chunks to the left (updated). Returns
// the 4 integral entries of the lane's columns: column c holds the sum of the entries < c, {prev lane's last, P0, P1, P2}.
__device__ __forceinline__ uint4 row_prefix_u32(const unsigned (&p)[4], unsigned& carry, int lane) {
  const unsigned a0 = p[0], a1 = a0 + p[1], a2 = a1 + p[2], a3 = a2 + p[3];
  const unsigned base = carry + wave_scan_u32(a3) - a3;
  const unsigned last = base + a3;
  unsigned prev = dpp_u32<0x138, 0xF>(last);  // wave_shr:1: value of the previous lane
  if (lane == 0) prev = carry;
  carry = (unsigned)__builtin_amdgcn_readlane((int)last, 63);
  return make_uint4(prev, base + a0, base + a1, base + a2);
}

template <bool SQ>
__global__ __launch_bounds__(256) void k_integral_band(const uint8_t* __restrict__ pyr, size_t pyr_frame_bytes,
                                                       int32_t* __restrict__ integ, size_t int_frame_elems, int nchan,
                                                       const int32_t* __restrict__ hbuf, size_t h_frame_elems,
                                                       const ScaleDev* __restrict__ sd, int nscales,
                                                       const int* __restrict__ band_first, int total_bands, int sq_odd_rows_only) {
  const int lane = threadIdx.x & 63;
  const int gb = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gb >= total_bands) return;
  const int s = find_segment(band_first, nscales, gb);
  const ScaleDev S = sd[s];
  const int bnd = gb - band_first[s];
  const int r0 = bnd * INT_BAND;
  const int nrows = min(INT_BAND, S.h - r0);
  const size_t f = blockIdx.y;
  const uint8_t* src = pyr + f * pyr_frame_bytes + S.img_ofs + (size_t)r0 * S.pitch8;
  int32_t* osum = integ + (f * nchan + 0) * int_frame_elems + S.int_ofs + (size_t)(r0 + 1) * S.pitchI;
  int32_t* osq = SQ ? integ + (f * nchan + 1) * int_frame_elems + S.int_ofs + (size_t)(r0 + 1) * S.pitchI : nullptr;
  const int32_t* hsum = hbuf + (f * nchan + 0) * h_frame_elems + S.h_ofs + (size_t)bnd * S.pitchI;
  const int32_t* hsq = SQ ? hbuf + (f * nchan + 1) * h_frame_elems + S.h_ofs + (size_t)bnd * S.pitchI : nullptr;
  unsigned carry_s[INT_BAND], carry_q[INT_BAND];
#pragma unroll
  for (int r = 0; r < INT_BAND; r++) carry_s[r] = carry_q[r] = 0;
  unsigned carry_hs = 0, carry_hq = 0;
  for (int c0 = 0; c0 < S.pitchI; c0 += 256) {
    const int px = c0 + lane * 4;
    const bool col_ok = px < S.pitchI;
    uint4 vs = make_uint4(0, 0, 0, 0), vq = make_uint4(0, 0, 0, 0);  // running vertical sums of the row prefixes
    if (bnd == 0) {  // no rows above; integral row 0 is all zeros
      if (col_ok) {
        *reinterpret_cast<int4*>(osum - S.pitchI + px) = make_int4(0, 0, 0, 0);
        if (SQ) *reinterpret_cast<int4*>(osq - S.pitchI + px) = make_int4(0, 0, 0, 0);
      }
    } else {  // the rows above this band: the column sums of the bands above it go through the scan like a row of pixels
      int4 a = make_int4(0, 0, 0, 0), q = make_int4(0, 0, 0, 0);
      if (col_ok) {
        a = *reinterpret_cast<const int4*>(hsum + px);
        if (SQ) q = *reinterpret_cast<const int4*>(hsq + px);
      }
      const unsigned ha[4] = {(unsigned)a.x, (unsigned)a.y, (unsigned)a.z, (unsigned)a.w};
      vs = row_prefix_u32(ha, carry_hs, lane);
      if (SQ) {
        const unsigned hq[4] = {(unsigned)q.x, (unsigned)q.y, (unsigned)q.z, (unsigned)q.w};
        vq = row_prefix_u32(hq, carry_hq, lane);
      }
    }
    unsigned word[INT_BAND];
#pragma unroll
    for (int r = 0; r < INT_BAND; r++)
      word[r] = (r < nrows && px < S.pitch8) ? *reinterpret_cast<const unsigned*>(src + (size_t)r * S.pitch8 + px) : 0u;
#pragma unroll
    for (int r = 0; r < INT_BAND; r++) {
      unsigned p[4], pp[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        p[k] = (px + k < S.w) ? ((word[r] >> (8 * k)) & 0xffu) : 0u;
        pp[k] = p[k] * p[k];
      }
      const uint4 rs = row_prefix_u32(p, carry_s[r], lane);
      vs.x += rs.x;
      vs.y += rs.y;
      vs.z += rs.z;
      vs.w += rs.w;
      if (SQ) {
        const uint4 rq = row_prefix_u32(pp, carry_q[r], lane);
        vq.x += rq.x;
        vq.y += rq.y;
        vq.z += rq.z;
        vq.w += rq.w;
      }
      if (col_ok && r < nrows) {
        *reinterpret_cast<int4*>(osum + (size_t)r * S.pitchI + px) = make_int4((int)vs.x, (int)vs.y, (int)vs.z, (int)vs.w);
        // The detector reads the squared sums only at the 4 corners of each window's variance rectangle: with a scan
        // step of 2 and an even window height those are odd integral rows; the even rows are never read, so they are
        // not written
        if (SQ) {
          if (sq_odd_rows_only && S.ystep == 2) {
            // ... and of those rows only the odd columns, which are packed (column 2c+1 at c): 8 bytes per lane
            if ((r0 + 1 + r) & 1) *reinterpret_cast<int2*>(osq + (size_t)r * S.pitchI + (px >> 1)) = make_int2((int)vq.y, (int)vq.w);
          } else
            *reinterpret_cast<int4*>(osq + (size_t)r * S.pitchI + px) = make_int4((int)vq.x, (int)vq.y, (int)vq.z, (int)vq.w);
        }
      }
    }
  }
}

// Column sums of the bands of levels the caller filled in itself (no k_resize ran): block = one band of one scale,
// thread = 4 adjacent columns, vertical adds only. Same output as k_resize's: H[b][x] per pixel column, 0 from w to pitchI.
template <bool SQ>
__global__ __launch_bounds__(256) void k_band_colsums(const uint8_t* __restrict__ pyr, size_t pyr_frame_bytes, int nchan,
                                                      int32_t* __restrict__ hbuf, size_t h_frame_elems,
                                                      const ScaleDev* __restrict__ sd, int nscales,
                                                      const int* __restrict__ band_first) {
  const int s = find_segment(band_first, nscales, blockIdx.x);
  const ScaleDev S = sd[s];
  const int bnd = blockIdx.x - band_first[s];
  const int r0 = bnd * INT_BAND;
  const int nrows = min(INT_BAND, S.h - r0);
  const size_t f = blockIdx.y;
  const uint8_t* src = pyr + f * pyr_frame_bytes + S.img_ofs + (size_t)r0 * S.pitch8;
  int32_t* hsum = hbuf + (f * nchan + 0) * h_frame_elems + S.h_ofs + (size_t)bnd * S.pitchI;
  int32_t* hsq = SQ ? hbuf + (f * nchan + 1) * h_frame_elems + S.h_ofs + (size_t)bnd * S.pitchI : nullptr;
  for (int px = threadIdx.x * 4; px < S.pitchI; px += 1024) {
    unsigned cs[4] = {0, 0, 0, 0}, cq[4] = {0, 0, 0, 0};
    if (px < S.pitch8)
      for (int r = 0; r < nrows; r++) {
        const unsigned word = *reinterpret_cast<const unsigned*>(src + (size_t)r * S.pitch8 + px);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const unsigned v = (px + k < S.w) ? ((word >> (8 * k)) & 0xffu) : 0u;
          cs[k] += v;
          cq[k] += v * v;
        }
      }
    *reinterpret_cast<int4*>(hsum + px) = make_int4((int)cs[0], (int)cs[1], (int)cs[2], (int)cs[3]);
    if (SQ) *reinterpret_cast<int4*>(hsq + px) = make_int4((int)cq[0], (int)cq[1], (int)cq[2], (int)cq[3]);
  }
}

// Exclusive scan of the band totals down the bands (in place): thread = 4 adjacent columns of one channel of one scale.
__global__ __launch_bounds__(64) void k_integral_carry(int32_t* __restrict__ hbuf, size_t h_frame_elems, int nchan,
                                                       const ScaleDev* __restrict__ sd, int nscales,
                                                       const int* __restrict__ blk_first) {
  const int s = find_segment(blk_first, nscales, blockIdx.x);
  const ScaleDev S = sd[s];
  const int quad = (blockIdx.x - blk_first[s]) * 64 + threadIdx.x;
  if (quad * 4 >= S.pitchI) return;
  int4* p = reinterpret_cast<int4*>(hbuf + ((size_t)blockIdx.y * nchan + blockIdx.z) * h_frame_elems + S.h_ofs) + quad;
  const size_t pitch4 = S.pitchI >> 2;
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (int b = 0; b < S.nbands; b++) {
    const int4 v = p[(size_t)b * pitch4];
    p[(size_t)b * pitch4] = make_int4((int)acc.x, (int)acc.y, (int)acc.z, (int)acc.w);
    acc.x += (unsigned)v.x;
    acc.y += (unsigned)v.y;
    acc.z += (unsigned)v.z;
    acc.w += (unsigned)v.w;
  }
}

// ------------------------------------------------------------------------------------------------
// Tilted (45 degree) integral for whole pyramid levels, needed only by cascades with tilted Haar features.
// With L(y,x) = sum of the pixels on the diagonal going up-left from (y-1, x) and R(y,x) = the same going up-right,
//   tilted(y, x) = tilted(y-1, x) + p(y-1, x-1) + L(y-1, x-2) + R(y-1, x)
// (the new bottom pixel of the triangle plus its two new edges), a plain column recurrence; L and R are prefix sums
// along diagonals: L(y,x) = L(y-1,x-1) + p(y-1,x), R(y,x) = R(y-1,x+1) + p(y-1,x). Pixels outside the image are 0, so
// every recurrence is border-safe.
// All three are running sums along y. Round 2 gave a whole diagonal / column to one thread: 1 080 dependent steps for a
// Full-HD image and only w + h threads per scale. Now the y axis is cut into segments of TSEG rows and each sum runs in
// two passes, like the band integrals: the *_totals kernels add up a segment (thread = one diagonal or column of one
// segment), the second kernel starts from the totals of the segments above it (at most h / TSEG small reads) and writes
// the segment's running sums. ~17x the threads for Full-HD, 64 + 17 dependent steps instead of 1 080.
// ------------------------------------------------------------------------------------------------
constexpr int TSEG = 64;  // rows per segment

// Layout of the segment totals of one frame, per scale s at tseg_ofs[s]: L totals [nseg][w + h - 1], R totals likewise,
// then the column totals of the tilted recurrence [nseg][w + 1].
struct TiltSegs {
  int nseg, ndiag, ncol;
  __host__ __device__ TiltSegs(int w, int h) : nseg((h + TSEG - 1) / TSEG), ndiag(w + h - 1), ncol(w + 1) {}
  __host__ __device__ size_t elems() const { return (size_t)nseg * (2 * (size_t)ndiag + (size_t)ncol); }
  __host__ __device__ size_t diag_at(int dir, int g) const { return ((size_t)dir * nseg + g) * (size_t)ndiag; }
  __host__ __device__ size_t col_at(int g) const { return 2 * (size_t)nseg * ndiag + (size_t)g * ncol; }
};

// A block is TILT_GROUPS wavefronts, each with its own group of 64 adjacent diagonals (or columns). Measured (16 Full-HD
// frames, rocprofv3): 1 group per block 2.41 ms for the four kernels, 4 groups per block 2.64 ms -- making the 256-byte
// pieces of neighbouring groups leave one CU together does not help, fewer and fatter blocks schedule worse.
constexpr int TILT_GROUPS = 1;
// group = 64 threads = 256 adjacent diagonals of one scale (a thread walks 4 of them: their pixels are 4 consecutive bytes
// of a row -- one unaligned 32-bit load -- and their sums 4 consecutive words of the output row -- one 16-byte store);
// blockIdx.y = frame, z = 2 * segment + direction (0: L, x - y constant; 1: R, x + y constant)
struct __attribute__((packed, aligned(1))) Bytes4 {
  unsigned d;
};
struct __attribute__((packed, aligned(4))) Words4 {
  int d[4];
};
template <bool FINAL>
__global__ __launch_bounds__(64 * TILT_GROUPS) void k_diag_sums(const uint8_t* __restrict__ pyr, size_t pyr_frame_bytes, int32_t* __restrict__ diag,
                                                  size_t int_frame_elems, int32_t* __restrict__ tseg, size_t tseg_frame_elems,
                                                  const long long* __restrict__ tseg_ofs, const ScaleDev* __restrict__ sd, int nscales,
                                                  const int* __restrict__ blk_first, int n_groups) {
  const int grp = blockIdx.x * TILT_GROUPS + (threadIdx.x >> 6);
  if (grp >= n_groups) return;
  const int s = find_segment(blk_first, nscales, grp);
  const ScaleDev S = sd[s];
  const TiltSegs T(S.w, S.h);
  const int t = ((grp - blk_first[s]) * 64 + (threadIdx.x & 63)) * 4;  // first of this thread's 4 diagonals
  const int dir = blockIdx.z & 1, g = blockIdx.z >> 1;
  if (t >= T.ndiag || g >= T.nseg) return;
  const uint8_t* img = pyr + (size_t)blockIdx.y * pyr_frame_bytes + S.img_ofs;
  int32_t* tot = tseg + (size_t)blockIdx.y * tseg_frame_elems + tseg_ofs[s];
  const int d = dir ? t : t - (S.h - 1);
  const int y0 = g * TSEG, y1 = min(y0 + TSEG, S.h);
  int acc[4] = {0, 0, 0, 0};
  if (FINAL)
    for (int k = 0; k < g; k++)  // the segments above this one
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (t + j < T.ndiag) acc[j] += tot[T.diag_at(dir, k) + t + j];
  int32_t* out = diag + ((size_t)blockIdx.y * 2 + dir) * int_frame_elems + S.int_ofs;
  for (int y = y0; y < y1; y++) {
    const int x = dir ? d - y : d + y;  // column of the first diagonal; the other three follow
    if (x >= 0 && x + 3 < S.w) {
      const unsigned px = reinterpret_cast<const Bytes4*>(img + (size_t)y * S.pitch8 + x)->d;
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] += (int)((px >> (8 * j)) & 0xffu);
      if (FINAL) *reinterpret_cast<Words4*>(out + (size_t)(y + 1) * S.pitchI + x) = Words4{{acc[0], acc[1], acc[2], acc[3]}};
    } else if (x + 3 >= 0 && x < S.w) {  // the image border cuts the group
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (x + j >= 0 && x + j < S.w) {
          acc[j] += img[(size_t)y * S.pitch8 + x + j];
          if (FINAL) out[(size_t)(y + 1) * S.pitchI + x + j] = acc[j];
        }
    }
  }
  if (!FINAL)
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (t + j < T.ndiag) tot[T.diag_at(dir, g) + t + j] = acc[j];
}

// group = 64 columns of one scale; blockIdx.y = frame, z = segment (rows y0 + 1 .. y1 of the tilted integral)
template <bool FINAL>
__global__ __launch_bounds__(64 * TILT_GROUPS) void k_tilted_cols(const uint8_t* __restrict__ pyr, size_t pyr_frame_bytes,
                                                    const int32_t* __restrict__ diag, int32_t* __restrict__ integ,
                                                    size_t int_frame_elems, int nchan, int tilt_chan, int32_t* __restrict__ tseg,
                                                    size_t tseg_frame_elems, const long long* __restrict__ tseg_ofs,
                                                    const ScaleDev* __restrict__ sd, int nscales, const int* __restrict__ blk_first,
                                                    int n_groups) {
  const int grp = blockIdx.x * TILT_GROUPS + (threadIdx.x >> 6);
  if (grp >= n_groups) return;
  const int s = find_segment(blk_first, nscales, grp);
  const ScaleDev S = sd[s];
  const TiltSegs Tg(S.w, S.h);
  const int x = (grp - blk_first[s]) * 64 + (threadIdx.x & 63);
  const int g = blockIdx.z;
  if (x > S.w || g >= Tg.nseg) return;
  const uint8_t* img = pyr + (size_t)blockIdx.y * pyr_frame_bytes + S.img_ofs;
  const int32_t* L = diag + ((size_t)blockIdx.y * 2 + 0) * int_frame_elems + S.int_ofs;
  const int32_t* R = diag + ((size_t)blockIdx.y * 2 + 1) * int_frame_elems + S.int_ofs;
  int32_t* T = integ + ((size_t)blockIdx.y * nchan + tilt_chan) * int_frame_elems + S.int_ofs;
  int32_t* tot = tseg + (size_t)blockIdx.y * tseg_frame_elems + tseg_ofs[s];
  const int y0 = g * TSEG + 1, y1 = min(y0 + TSEG - 1, S.h);  // integral rows of this segment
  int acc = 0;
  if (FINAL) {
    for (int k = 0; k < g; k++) acc += tot[Tg.col_at(k) + x];
    if (g == 0) T[x] = 0;  // row 0
  }
  for (int y = y0; y <= y1; y++) {
    int v = x >= 1 ? img[(size_t)(y - 1) * S.pitch8 + (x - 1)] : 0;
    if (y >= 2) {
      if (x >= 2) v += L[(size_t)(y - 1) * S.pitchI + (x - 2)];
      if (x < S.w) v += R[(size_t)(y - 1) * S.pitchI + x];
    }
    acc += v;
    if (FINAL) T[(size_t)y * S.pitchI + x] = acc;
  }
  if (!FINAL) tot[Tg.col_at(g) + x] = acc;
}

// ------------------------------------------------------------------------------------------------
// K0: colour -> gray (COLOR_BGR2GRAY's integer form, include/cascadeclassifier_amd.h), in front of the pyramid: the gray
// frames land in the detector's staging slots with the layout stage_host_frames gives gray frames, so everything behind
// this kernel is the gray path unchanged. Memory-bound (3-4 bytes in, 1 out per pixel): a lane takes 16 pixels of a row,
// reads them with 16-byte loads at whatever alignment the row has (3 or 4 of them interleaved, one per plane for the
// planar format) and writes one 16-byte store. A row's last width % 16 pixels go byte by byte, by one lane of the row.
// ------------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(4))) Gray16 {  // 16 gray bytes at a multiple of 4 (the staging layout's pitch)
  unsigned d[4];
};
__device__ __forceinline__ unsigned gray_of(unsigned b, unsigned g, unsigned r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }
template <int FMT>
__global__ __launch_bounds__(256) void k_to_gray(const uint8_t* __restrict__ src, size_t row_stride, size_t frame_stride, int w, int h,
                                                 int chunks_per_row, uint8_t* __restrict__ dst, size_t dst_stride, size_t dst_frame_stride) {
  constexpr bool PLANAR = FMT == CC_PIX_RGB8_PLANAR;
  constexpr int BPP = (FMT == CC_PIX_BGR8 || FMT == CC_PIX_RGB8) ? 3 : (FMT == CC_PIX_BGRA8 || FMT == CC_PIX_RGBA8) ? 4 : 1;
  // byte of a pixel (planar: plane) that holds B and R; G is byte 1
  constexpr int CB = (FMT == CC_PIX_BGR8 || FMT == CC_PIX_BGRA8) ? 0 : (FMT == CC_PIX_GRAY8 ? 0 : 2);
  constexpr int CR = (FMT == CC_PIX_BGR8 || FMT == CC_PIX_BGRA8) ? 2 : 0;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int y = i / chunks_per_row;
  if (y >= h) return;
  const int x0 = (i - y * chunks_per_row) * 16;
  const uint8_t* s = src + (size_t)blockIdx.y * frame_stride + (size_t)y * row_stride;
  const size_t plane = row_stride * (size_t)h;
  uint8_t* o = dst + (size_t)blockIdx.y * dst_frame_stride + (size_t)y * dst_stride + x0;
  auto px = [&](int x, int c) -> unsigned {  // channel c of pixel x, one byte load
    if (FMT == CC_PIX_GRAY8) return s[x];
    return PLANAR ? s[(size_t)c * plane + x] : s[(size_t)x * BPP + c];
  };
  if (x0 + 16 <= w) {
    constexpr int NW = PLANAR ? 12 : 4 * BPP;  // words loaded
    unsigned v[NW];
    if (PLANAR) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const Bytes16 q = *reinterpret_cast<const Bytes16*>(s + (size_t)c * plane + x0);
#pragma unroll
        for (int j = 0; j < 4; j++) v[4 * c + j] = q.d[j];
      }
    } else {
#pragma unroll
      for (int k = 0; k < BPP; k++) {
        const Bytes16 q = *reinterpret_cast<const Bytes16*>(s + (size_t)x0 * BPP + 16 * k);
#pragma unroll
        for (int j = 0; j < 4; j++) v[4 * k + j] = q.d[j];
      }
    }
    // byte n of the loaded words: interleaved pixel k channel c at n = BPP k + c; planar plane c pixel k at n = 16 c + k
    auto byte = [&](int n) -> unsigned { return (v[n >> 2] >> (8 * (n & 3))) & 255u; };
    Gray16 g;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned word = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int k = 4 * j + b;
        unsigned gv;
        if (FMT == CC_PIX_GRAY8)
          gv = byte(k);
        else if (PLANAR)
          gv = gray_of(byte(32 + k), byte(16 + k), byte(k));
        else
          gv = gray_of(byte(BPP * k + CB), byte(BPP * k + 1), byte(BPP * k + CR));
        word |= gv << (8 * b);
      }
      g.d[j] = word;
    }
    *reinterpret_cast<Gray16*>(o) = g;
  } else {
    for (int x = x0; x < w; x++)
      o[x - x0] = FMT == CC_PIX_GRAY8 ? (uint8_t)px(x, 0) : (uint8_t)gray_of(px(x, CB), px(x, 1), px(x, CR));
  }
}

void launch_to_gray(hipStream_t st, int fmt, const uint8_t* src, size_t row_stride, size_t frame_stride, int w, int h, int nf,
                    uint8_t* dst, size_t dst_stride, size_t dst_frame_stride) {
  if (nf <= 0 || w <= 0 || h <= 0) return;
  const int cpr = (w + 15) / 16;
  const dim3 grid((unsigned)(((long long)h * cpr + 255) / 256), (unsigned)nf);
#define CC_TO_GRAY(F)                                                                                                     \
  case F:                                                                                                                  \
    hipLaunchKernelGGL(k_to_gray<F>, grid, dim3(256), 0, st, src, row_stride, frame_stride, w, h, cpr, dst, dst_stride, \
                       dst_frame_stride);                                                                                  \
    break;
  switch (fmt) {
    CC_TO_GRAY(CC_PIX_GRAY8)
    CC_TO_GRAY(CC_PIX_BGR8)
    CC_TO_GRAY(CC_PIX_BGRA8)
    CC_TO_GRAY(CC_PIX_RGB8)
    CC_TO_GRAY(CC_PIX_RGBA8)
    CC_TO_GRAY(CC_PIX_RGB8_PLANAR)
    default: break;
  }
#undef CC_TO_GRAY
}

FrontLayout front_layout(int src_w, int src_h, const std::vector<int2>& sizes, bool tilted) {
  const int ns = (int)sizes.size();
  FrontLayout L;
  L.src_w = src_w;
  L.src_h = src_h;
  L.sd.resize(ns);
  for (std::vector<int>* v : {&L.resize_first, &L.band_first, &L.col_first, &L.diag_first, &L.tcol_first}) v->assign(ns + 1, 0);
  if (tilted) L.tseg_ofs.assign(ns + 1, 0);
  long long img_ofs = 0, int_ofs = 0, h_ofs = 0;
  for (int i = 0; i < ns; i++) {
    ScaleDev& S = L.sd[i];
    S.w = sizes[i].x;
    S.h = sizes[i].y;
    S.pitch8 = align_up(S.w, 4);
    S.pitchI = align_up(S.w + 1, 4);
    S.img_ofs = img_ofs;
    S.int_ofs = int_ofs;
    S.h_ofs = h_ofs;
    S.nbands = (S.h + INT_BAND - 1) / INT_BAND;
    AxisTaps tx, ty;
    linear_exact_taps(src_w, S.w, tx);
    linear_exact_taps(src_h, S.h, ty);
    S.xtab_ofs = append_column_taps(tx, L.xofs, L.xw1);
    S.ytab_ofs = (int)L.yofs.size();
    L.yofs.insert(L.yofs.end(), ty.ofs.begin(), ty.ofs.end());
    L.yw1.insert(L.yw1.end(), ty.w1.begin(), ty.w1.end());
    img_ofs += (long long)align_up(S.pitch8 * S.h, 16);
    int_ofs += (long long)S.pitchI * (S.h + 1);
    h_ofs += (long long)S.nbands * S.pitchI;
    L.resize_first[i + 1] = L.resize_first[i] + resize_blocks(S.pitch8, S.h);
    L.band_first[i + 1] = L.band_first[i] + S.nbands;
    L.col_first[i + 1] = L.col_first[i] + (S.pitchI / 4 + 63) / 64;
    L.diag_first[i + 1] = L.diag_first[i] + (S.w + S.h - 1 + 255) / 256;  // k_diag_sums: a thread walks 4 diagonals
    L.tcol_first[i + 1] = L.tcol_first[i] + (S.w + 1 + 63) / 64;
    if (tilted) {
      const TiltSegs T(S.w, S.h);
      L.tseg_ofs[i + 1] = L.tseg_ofs[i] + (long long)T.elems();
      L.max_nseg = std::max(L.max_nseg, T.nseg);
    }
  }
  L.pyr_frame_bytes = (size_t)((img_ofs + 15) & ~15LL);
  L.int_frame_elems = (size_t)int_ofs;
  L.h_frame_elems = (size_t)h_ofs;
  if (tilted) L.tseg_frame_elems = (size_t)L.tseg_ofs[ns];
  return L;
}

void launch_front(hipStream_t st, const FrontTables& T, const FrontIO& io, int nf, int parts) {
  const FrontLayout& L = T.L;
  const int ns = (int)L.sd.size();
  if (ns == 0 || nf == 0) return;
  // io.hbuf set: the pyramid kernel also writes the column sums of the integral bands
  if (parts & FRONT_RESIZE)
    hipLaunchKernelGGL(k_resize, dim3(L.resize_first[ns], nf), dim3(256), 0, st, io.src, io.row_stride, io.frame_stride, L.src_w, L.src_h,
                       io.pyr, L.pyr_frame_bytes, T.d_sd.p, ns, T.d_resize_first.p, T.d_xofs.p, T.d_xw1.p, T.d_yofs.p, T.d_yw1.p, io.hbuf,
                       L.h_frame_elems, io.nchan, io.sq ? 1 : 0);
  if (!(parts & FRONT_INTEGRALS)) return;
  // integral images: band column sums (unless k_resize left them: see FrontIO::src), carry down the bands, finished integral
  const int n_bands = L.band_first[ns];
  if (!io.src) {
    if (io.sq)
      hipLaunchKernelGGL(k_band_colsums<true>, dim3(n_bands, nf), dim3(256), 0, st, io.pyr, L.pyr_frame_bytes, io.nchan, io.hbuf,
                         L.h_frame_elems, T.d_sd.p, ns, T.d_band_first.p);
    else
      hipLaunchKernelGGL(k_band_colsums<false>, dim3(n_bands, nf), dim3(256), 0, st, io.pyr, L.pyr_frame_bytes, io.nchan, io.hbuf,
                         L.h_frame_elems, T.d_sd.p, ns, T.d_band_first.p);
  }
  hipLaunchKernelGGL(k_integral_carry, dim3(L.col_first[ns], nf, io.sq ? 2 : 1), dim3(64), 0, st, io.hbuf, L.h_frame_elems, io.nchan, T.d_sd.p,
                     ns, T.d_col_first.p);
  const dim3 grid((n_bands + 3) / 4, nf);
  if (io.sq)
    hipLaunchKernelGGL(k_integral_band<true>, grid, dim3(256), 0, st, io.pyr, L.pyr_frame_bytes, io.integ, L.int_frame_elems, io.nchan,
                       io.hbuf, L.h_frame_elems, T.d_sd.p, ns, T.d_band_first.p, n_bands, io.sq_odd_rows_only);
  else
    hipLaunchKernelGGL(k_integral_band<false>, grid, dim3(256), 0, st, io.pyr, L.pyr_frame_bytes, io.integ, L.int_frame_elems, io.nchan,
                       io.hbuf, L.h_frame_elems, T.d_sd.p, ns, T.d_band_first.p, n_bands, io.sq_odd_rows_only);
  if (L.max_nseg == 0) return;
  // tilted integral into channel tilt_chan: diagonal sums, then the column recurrence, each as segment totals + final pass
  const int n_diag = L.diag_first[ns], n_tcol = L.tcol_first[ns];
  const dim3 gd((n_diag + TILT_GROUPS - 1) / TILT_GROUPS, nf, 2 * L.max_nseg), gc((n_tcol + TILT_GROUPS - 1) / TILT_GROUPS, nf, L.max_nseg);
  const dim3 bt(64 * TILT_GROUPS);
  hipLaunchKernelGGL(k_diag_sums<false>, gd, bt, 0, st, io.pyr, L.pyr_frame_bytes, io.diag, L.int_frame_elems, io.tseg, L.tseg_frame_elems,
                     T.d_tseg_ofs.p, T.d_sd.p, ns, T.d_diag_first.p, n_diag);
  hipLaunchKernelGGL(k_diag_sums<true>, gd, bt, 0, st, io.pyr, L.pyr_frame_bytes, io.diag, L.int_frame_elems, io.tseg, L.tseg_frame_elems,
                     T.d_tseg_ofs.p, T.d_sd.p, ns, T.d_diag_first.p, n_diag);
  hipLaunchKernelGGL(k_tilted_cols<false>, gc, bt, 0, st, io.pyr, L.pyr_frame_bytes, io.diag, io.integ, L.int_frame_elems, io.nchan, io.tilt_chan,
                     io.tseg, L.tseg_frame_elems, T.d_tseg_ofs.p, T.d_sd.p, ns, T.d_tcol_first.p, n_tcol);
  hipLaunchKernelGGL(k_tilted_cols<true>, gc, bt, 0, st, io.pyr, L.pyr_frame_bytes, io.diag, io.integ, L.int_frame_elems, io.nchan, io.tilt_chan,
                     io.tseg, L.tseg_frame_elems, T.d_tseg_ofs.p, T.d_sd.p, ns, T.d_tcol_first.p, n_tcol);
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_resize_linear_exact_u8(int device, const uint8_t* src, int sw, int sh, size_t sstride, uint8_t* dst, int dw, int dh,
                                    size_t dstride) {
  if (!src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || sstride < (size_t)sw || dstride < (size_t)dw)
    return set_error(CC_ERR_INVALID_ARG, "cc_resize_linear_exact_u8: bad argument");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  FrontTables T;
  T.L = front_layout(sw, sh, {make_int2(dw, dh)}, false);
  CC_HIP(T.upload(own.s));
  DevBuf<uint8_t> d_src, d_dst;
  const size_t spitch = (size_t)align_up(sw, 4);
  CC_HIP(d_src.ensure(spitch * sh));
  CC_HIP(d_dst.ensure(T.L.pyr_frame_bytes));
  CC_HIP(hipMemcpy2DAsync(d_src.p, spitch, src, sstride, sw, sh, hipMemcpyHostToDevice, own.s));
  FrontIO io;
  io.src = d_src.p;
  io.row_stride = spitch;
  io.pyr = d_dst.p;
  launch_front(own.s, T, io, 1, FRONT_RESIZE);
  CC_HIP(hipGetLastError());
  CC_HIP(hipMemcpy2DAsync(dst, dstride, d_dst.p, T.L.sd[0].pitch8, dw, dh, hipMemcpyDeviceToHost, own.s));
  CC_HIP(hipStreamSynchronize(own.s));
  return CC_OK;
}

cc_status cc_integral_u8(int device, const uint8_t* img, int width, int height, size_t row_stride, int32_t* sum, int32_t* sqsum,
                         int32_t* tilted) {
  if (!img || width < 1 || height < 1 || row_stride < (size_t)width) return set_error(CC_ERR_INVALID_ARG, "cc_integral_u8: bad argument");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  FrontTables T;  // one level: the image itself, no resize
  T.L = front_layout(width, height, {make_int2(width, height)}, tilted != nullptr);
  CC_HIP(T.upload(own.s));
  const FrontLayout& L = T.L;
  const int nchan = tilted ? 3 : 2;  // sum, sqsum, tilted (same kernels as the detection pipeline)
  DevBuf<uint8_t> d_img;
  DevBuf<int32_t> d_int, d_h, d_diag, d_tseg;
  CC_HIP(d_img.ensure(L.pyr_frame_bytes));
  CC_HIP(d_int.ensure(L.int_frame_elems * nchan));
  CC_HIP(d_h.ensure(L.h_frame_elems * nchan));
  if (tilted) {
    CC_HIP(d_diag.ensure(L.int_frame_elems * 2));
    CC_HIP(d_tseg.ensure(std::max<size_t>(L.tseg_frame_elems, 1)));
  }
  CC_HIP(hipMemcpy2DAsync(d_img.p, L.sd[0].pitch8, img, row_stride, width, height, hipMemcpyHostToDevice, own.s));
  FrontIO io;
  io.pyr = d_img.p;
  io.integ = d_int.p;
  io.hbuf = d_h.p;
  io.diag = d_diag.p;
  io.tseg = d_tseg.p;
  io.nchan = nchan;
  io.sq = true;
  launch_front(own.s, T, io, 1, FRONT_INTEGRALS);
  CC_HIP(hipGetLastError());
  const size_t opitch = (size_t)(width + 1) * 4;
  int32_t* const out[3] = {sum, sqsum, tilted};
  for (int c = 0; c < nchan; c++)
    if (out[c])
      CC_HIP(hipMemcpy2DAsync(out[c], opitch, d_int.p + c * L.int_frame_elems, (size_t)L.sd[0].pitchI * 4, opitch, height + 1,
                              hipMemcpyDeviceToHost, own.s));
  CC_HIP(hipStreamSynchronize(own.s));
  return CC_OK;
}

cc_status cc_to_gray_u8(int device, const uint8_t* src, int pixel_format, int width, int height, size_t row_stride, uint8_t* dst,
                        size_t dst_stride) {
  const int bpp = pix_bytes(pixel_format);
  if (bpp == 0) return set_error(CC_ERR_INVALID_ARG, "cc_to_gray_u8: unknown pixel format %d", pixel_format);
  if (!src || !dst || width < 1 || height < 1 || row_stride < (size_t)width * bpp || dst_stride < (size_t)width)
    return set_error(CC_ERR_INVALID_ARG, "cc_to_gray_u8: bad argument");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  const int rows = pix_rows(pixel_format, height);
  const size_t span = (size_t)(rows - 1) * row_stride + (size_t)width * bpp;  // bytes from the first pixel to the last
  const size_t lead = (size_t)((uintptr_t)src & 15);  // the device copy starts at the same offset within 16 bytes
  const size_t dpitch = (size_t)align_up(width, 4);
  DevBuf<uint8_t> d_src, d_dst;
  CC_HIP(d_src.ensure(lead + span));
  CC_HIP(d_dst.ensure(dpitch * (size_t)height));
  CC_HIP(hipMemcpyAsync(d_src.p + lead, src, span, hipMemcpyHostToDevice, own.s));
  launch_to_gray(own.s, pixel_format, d_src.p + lead, row_stride, 0, width, height, 1, d_dst.p, dpitch, 0);
  CC_HIP(hipGetLastError());
  CC_HIP(hipMemcpy2DAsync(dst, dst_stride, d_dst.p, dpitch, width, height, hipMemcpyDeviceToHost, own.s));
  CC_HIP(hipStreamSynchronize(own.s));
  return CC_OK;
}

}  // extern "C"
