// ghx_addr.hpp — the address arithmetic of the segment and tile records (ghx_internal.hpp), in
// one copy for the gfx950 kernels and for host code that replays a plan (tests/cpp): the magic
// division, the general structured field offset, and the transformed tile's decode, offsets and
// negation predicate. Host-and-device under hipcc's HIP mode, plain inline otherwise. The short
// form field_offset_f stays with the kernels: its full-rate 24-bit products are device code.
#pragma once

#include "ghx_internal.hpp"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GHX_HD __host__ __device__ __forceinline__
#else
#define GHX_HD inline
#endif

namespace ghx
{
GHX_HD uint32_t fastdiv(uint32_t n, magic_u32 m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = __umulhi(m.m, n);
#else
    const uint32_t t = uint32_t((uint64_t(m.m) * n) >> 32);
#endif
    return (t + ((n - t) >> m.s1)) >> m.s2;
}

// field byte offset of segment-relative buffer position p (structured, general form)
GHX_HD int64_t field_offset_s(const seg_s& s, uint32_t p)
{
    const uint32_t row = fastdiv(p, s.mag_row);
    const uint32_t col = p - row * s.row_bytes;
    const uint32_t q0 = fastdiv(row, s.mag_ext[0]);
    const uint32_t c0 = row - q0 * s.ext[0];
    const uint32_t q1 = fastdiv(q0, s.mag_ext[1]);
    const uint32_t c1 = q0 - q1 * s.ext[1];
    const uint32_t q2 = fastdiv(q1, s.mag_ext[2]);
    const uint32_t c2 = q1 - q2 * s.ext[2];
    return s.field_off + int64_t(c0) * s.stride[0] + int64_t(c1) * s.stride[1] +
           int64_t(c2) * s.stride[2] + int64_t(q2) * s.stride[3] + int64_t(col);
}

// Adjoint accumulate tile (sacc_tile): the vectors a launch of width log2 w (<= s.wlog2) takes
// from it, and vector i's place: the outer coordinates c of its row and its byte column in the row.
// A planned vector (1 << wlog2 bytes) splits into 1 << (wlog2 - w) narrowed ones.
GHX_HD uint32_t sacc_vectors(const sacc_tile& s, int w) { return (s.n_rows * (s.len >> s.wlog2)) << (s.wlog2 - w); }

GHX_HD void sacc_decode(const sacc_tile& s, uint32_t i, int w, uint32_t (&c)[4], uint32_t& col)
{
    const int k = s.wlog2 - w;
    const uint32_t e = i >> k, sub = i & ((1u << k) - 1u);
    const uint32_t r = fastdiv(e, s.mag_vec);
    const uint32_t v = e - r * (s.len >> s.wlog2);
    col = s.col0 + (v << s.wlog2) + (sub << w);
    const uint32_t row = s.first_row + r;
    const uint32_t q0 = fastdiv(row, s.mag_ext[0]);
    c[0] = row - q0 * s.ext[0];
    const uint32_t q1 = fastdiv(q0, s.mag_ext[1]);
    c[1] = q0 - q1 * s.ext[1];
    c[3] = fastdiv(q1, s.mag_ext[2]);
    c[2] = q1 - c[3] * s.ext[2];
}

// the launch's vector width of a tile: the plan's, narrowed by the field pointer and by the buffer
// pointers the tile's sources read (mis8 / mis16: the slots whose pointer is not 8 / 16-B aligned)
GHX_HD int sacc_width(const sacc_tile& s, uint64_t field_ptr, uint64_t mis8, uint64_t mis16)
{
    int w = s.wlog2;
    if ((field_ptr & 15u) || (s.buf_mask & mis16)) w = w < 3 ? w : 3;
    if ((field_ptr & 7u) || (s.buf_mask & mis8)) w = w < 2 ? w : 2;
    return w;
}

// Coordinates of lane index i in a tile record's decode radix (tdim); false where they fall
// outside this tile's own extents (act: the last tile along an axis).
GHX_HD bool tile_decode(const seg_x& s, uint32_t i, uint32_t (&c)[4])
{
    const uint32_t q0 = fastdiv(i, s.mag[0]);
    c[0] = i - q0 * s.tdim[0];
    const uint32_t q1 = fastdiv(q0, s.mag[1]);
    c[1] = q0 - q1 * s.tdim[1];
    c[3] = fastdiv(q1, s.mag[2]);
    c[2] = q1 - c[3] * s.tdim[2];
    // one test after the three divisions (bitwise: no early exit between them)
    return bool(int(c[0] < s.act[0]) & int(c[1] < s.act[1]) & int(c[2] < s.act[2]) & int(c[3] < s.act[3]));
}

// off + sum c_k * stride_k: the receiving field's offset (seg_x::field_off, stride) or the
// sending field's (seg_xs::src_off, src_stride) of tile coordinates c. `off` is a byte offset
// or, in the kernels, the pointer that already includes it.
template<typename T>
GHX_HD T affine_offset(T off, const int64_t (&stride)[4], const uint32_t (&c)[4])
{
    return off + int64_t(c[0]) * stride[0] + int64_t(c[1]) * stride[1] + int64_t(c[2]) * stride[2] +
           int64_t(c[3]) * stride[3];
}

// element index of tile coordinates c in the buffer's dense box, from the tile's first cell
GHX_HD uint32_t tile_cell(const seg_x& s, const uint32_t (&c)[4])
{
    return c[0] * s.bstride[0] + c[1] * s.bstride[1] + c[2] * s.bstride[2] + c[3] * s.bstride[3];
}

// whether the element at tile coordinates c is a vector component that the transform negates
GHX_HD bool tile_negates(const seg_x& s, const uint32_t (&c)[4])
{
    const uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];  // plain locals: selects, no branches
    uint32_t comp = s.comp0;
    if (s.comp_pos < 4) comp += s.comp_pos == 0 ? c0 : s.comp_pos == 1 ? c1 : s.comp_pos == 2 ? c2 : c3;
    return comp < 2 && ((s.neg_mask >> comp) & 1u);
}
}  // namespace ghx
