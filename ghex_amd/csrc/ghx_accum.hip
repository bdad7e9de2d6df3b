// ghx_accum.hip — gfx950 (CDNA4) adjoint accumulate for index-list halos (k_accum_u and its get
// form k_accum_get_u) and, further down, for structured fields (k_accum_s, its get form
// k_accum_get_s and the cubed sphere's k_accum_get_x).
//
// The adjoint of the halo exchange sends every halo copy of a cell back to the cell's owner and
// sums it there. The contributions are already stored once: they are the message bytes a reverse
// pack (a ghx_uplan of direction 0 over the receive lists) left in the buffers. This kernel is the
// second pass: it sums per destination cell through an inverted index (uaccum_plan, ghx_accum_plan.cpp)
// whose lists keep a fixed order, so the result is bitwise reproducible. No atomics, no LDS.
//
// A workgroup takes one tile of destination rows of one field slot, a lane one element
// (destination d, level l): adjacent lanes take adjacent levels when a row's levels are adjacent
// in the field, adjacent destinations otherwise. The lane loads the destination's record range and
// lid, loads the cell, adds the contributions in record order — (entry, position) ascending — and
// stores the cell once. The loads of up to kAccBatch contributions are issued together (indices
// past the end clamped to the last record, their values not added), the adds stay in order: a
// destination of a real pattern has a handful of contributions (one per domain that holds the cell
// in its halo), so one trip serves it and no load waits for an earlier contribution's. A
// destination with ONE contribution, the most common, takes one load of each table and no clamped
// copies: the launch is bound by the load requests it issues (the duplicates cost 41 us of 203 at
// levels = 8), not by the latency of a lane's chain. Arithmetic
// is in the element type, integers as unsigned (they wrap). Zero tiles store zero bytes to their
// rows and load nothing from the field. All address arithmetic is 64-bit.
//
// This is the one file of the library that knows an element type. It is compiled without
// fast-math; the pragma below also keeps the compiler from contracting or reassociating.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "ghx_addr.hpp"
#include "ghx_internal.hpp"

#pragma clang fp contract(off) reassociate(off)

namespace ghx
{
// the calling thread's launch timing (ghx_kernels.hip, ghx_launch_timing)
extern thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>>* t_timing;

namespace
{
#define GHX_GLOBAL __attribute__((address_space(1)))

constexpr int kAccBatch = 4;  // contribution loads in flight per lane per trip

// table records are loaded as vectors of their words (one global_load each)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template<typename T>
__device__ __forceinline__ T load_contrib(const kargs_ua& a, uint32_t j, uint32_t l)
{
    const u32x2 c = ((const GHX_GLOBAL u32x2*)a.contribs)[j];  // entry, pos
    const GHX_GLOBAL u32x4* ep = (const GHX_GLOBAL u32x4*)(a.entries + c.x);
    const u32x4 e0 = ep[0];  // buf_off (2 words), n, levels
    const u32x4 e1 = ep[1];  // levels_first, buf_slot, pos_stride, lev_stride
    const uint64_t buf_off = uint64_t(e0.x) | (uint64_t(e0.y) << 32);
    const uint64_t elem = uint64_t(c.y) * e1.z + uint64_t(l) * e1.w;
    const char* p = reinterpret_cast<const char*>(a.buf_ptr[e1.y]) + buf_off + elem * sizeof(T);
    return *(const GHX_GLOBAL T*)(p);
}

// element e of a tile -> (row, level)
__device__ __forceinline__ void tile_element(const acc_tile& s, uint32_t e, uint32_t& r, uint32_t& l)
{
    if (s.lcontig)
    {
        r = fastdiv(e, s.mag);
        l = e - r * s.levels;
    }
    else
    {
        l = fastdiv(e, s.mag);
        r = e - l * s.n_rows;
    }
}

__device__ __forceinline__ int64_t dest_lid(const kargs_ua& a, uint32_t d)
{
    if (a.lid64) return ((const GHX_GLOBAL int64_t*)a.lids)[d];
    return ((const GHX_GLOBAL int32_t*)a.lids)[d];
}

template<typename T>
__device__ __forceinline__ void accum_tile(const kargs_ua& a, const acc_tile& s)
{
    char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]);
    const uint32_t ne = s.n_rows * s.levels;  // < 2^32 (planner)
    for (uint32_t e = threadIdx.x; e < ne; e += kBlock)
    {
        uint32_t r, l;
        tile_element(s, e, r, l);
        const uint32_t d = s.first_dest + r;
        const u32x2 rg = ((const GHX_GLOBAL u32x2*)a.ranges)[d];  // first, count
        const int64_t lid = dest_lid(a, d);
        GHX_GLOBAL T* cell = (GHX_GLOBAL T*)(field + lid * s.index_stride_b + int64_t(l) * s.level_stride_b);
        T acc = *cell;
        uint32_t j = rg.x, left = rg.y;
        if (left == 1)  // a cell with one halo copy, the common one: no clamped loads beside it
        {
            acc = T(acc + load_contrib<T>(a, j, l));
            left = 0;
        }
        while (left)
        {
            T v[kAccBatch];
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k) v[k] = load_contrib<T>(a, j + min(k, left - 1), l);
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k) acc = k < left ? T(acc + v[k]) : acc;
            const uint32_t step = min(uint32_t(kAccBatch), left);
            j += step;
            left -= step;
        }
        *cell = acc;
    }
}

template<typename T>
__device__ __forceinline__ void zero_tile(const kargs_ua& a, const acc_tile& s)
{
    char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]);
    const uint32_t ne = s.n_rows * s.levels;
    for (uint32_t e = threadIdx.x; e < ne; e += kBlock)
    {
        uint32_t r, l;
        tile_element(s, e, r, l);
        const int64_t lid = dest_lid(a, s.first_dest + r);
        *(GHX_GLOBAL T*)(field + lid * s.index_stride_b + int64_t(l) * s.level_stride_b) = T(0);
    }
}

__global__ __launch_bounds__(kBlock) void k_accum_u(kargs_ua a)
{
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const acc_tile s = a.tiles[t];
        const bool wide = s.dtype == GHX_DT_F64 || s.dtype == GHX_DT_I64;
        if (s.zero)
        {
            if (wide) zero_tile<uint64_t>(a, s);
            else zero_tile<uint32_t>(a, s);
        }
        else if (s.dtype == GHX_DT_F32) accum_tile<float>(a, s);
        else if (s.dtype == GHX_DT_F64) accum_tile<double>(a, s);
        else if (wide) accum_tile<uint64_t>(a, s);
        else accum_tile<uint32_t>(a, s);
    }
}

// ---------------------------------------------------------------------------------------------
// k_accum_get_u: k_accum_u's walk with a record's value taken from a buffer or, a field source,
// from the halo cell of a receiving field of the same launch (ghx_uaccum_get_create). The planner
// has resolved the source: the record holds the entry and an index `at` (message position or
// source lid), the entry the pointer slot and the element strides of `at` and of the level, so
// both kinds share one address form and the lane's chain stays record -> entry -> value. Wide:
// the plan's records are acc_get_rec64 (a source lid of 2^31 or more), one table per plan.
// The planner has verified that one record reads a halo cell and that nothing else touches it, so
// the lane that loaded it may store zero over it (zero_halos) with no other ordering.
// ---------------------------------------------------------------------------------------------
template<typename T, bool Wide>
__device__ __forceinline__ GHX_GLOBAL T* contrib_addr(const kargs_uag& a, uint32_t j, uint32_t l, uint32_t& field_src)
{
    uint32_t entry;
    uint64_t at;
    if constexpr (Wide)
    {
        const u32x4 c = ((const GHX_GLOBAL u32x4*)a.recs)[j];  // entry, pad, at (2 words)
        entry = c.x;
        at = uint64_t(c.z) | (uint64_t(c.w) << 32);
    }
    else
    {
        const u32x2 c = ((const GHX_GLOBAL u32x2*)a.recs)[j];  // entry, at
        entry = c.x;
        at = c.y;
    }
    const GHX_GLOBAL u32x4* ep = (const GHX_GLOBAL u32x4*)(a.entries + entry);
    const u32x4 e0 = ep[0];  // base (2 words), at_stride (2 words)
    const u32x4 e1 = ep[1];  // lev_stride (2 words), tab, field_src
    const uint64_t base = uint64_t(e0.x) | (uint64_t(e0.y) << 32);
    const uint64_t at_stride = uint64_t(e0.z) | (uint64_t(e0.w) << 32);
    const uint64_t lev_stride = uint64_t(e1.x) | (uint64_t(e1.y) << 32);
    field_src = e1.w;
    const uint64_t elem = at * at_stride + uint64_t(l) * lev_stride;  // mod 2^64: strides are signed
    return (GHX_GLOBAL T*)(reinterpret_cast<char*>(a.ptr[e1.z]) + base + elem * sizeof(T));
}

template<typename T, bool Wide>
__device__ __forceinline__ void accum_get_tile(const kargs_uag& a, const acc_tile& s)
{
    char* field = reinterpret_cast<char*>(a.ptr[s.field_slot]);
    const uint32_t ne = s.n_rows * s.levels;  // < 2^32 (planner)
    for (uint32_t e = threadIdx.x; e < ne; e += kBlock)
    {
        uint32_t r, l;
        tile_element(s, e, r, l);
        const uint32_t d = s.first_dest + r;
        const u32x2 rg = ((const GHX_GLOBAL u32x2*)a.ranges)[d];  // first, count
        const int64_t lid = a.lid64 ? ((const GHX_GLOBAL int64_t*)a.lids)[d] : ((const GHX_GLOBAL int32_t*)a.lids)[d];
        GHX_GLOBAL T* cell = (GHX_GLOBAL T*)(field + lid * s.index_stride_b + int64_t(l) * s.level_stride_b);
        T acc = *cell;
        uint32_t j = rg.x, left = rg.y;
        if (left == 1)  // a cell with one halo copy, the common one: no clamped loads beside it
        {
            uint32_t fs;
            GHX_GLOBAL T* p = contrib_addr<T, Wide>(a, j, l, fs);
            const T v = *p;
            if (a.zero_src & fs) *p = T(0);
            acc = T(acc + v);
            left = 0;
        }
        while (left)
        {
            GHX_GLOBAL T* p[kAccBatch];
            uint32_t fs[kAccBatch];
            T v[kAccBatch];
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k)
            {
                p[k] = contrib_addr<T, Wide>(a, j + min(k, left - 1), l, fs[k]);
                v[k] = *p[k];
            }
            // zero over the field sources this trip adds; a clamped copy past the end is neither
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k)
                if (k < left && (a.zero_src & fs[k])) *p[k] = T(0);
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k) acc = k < left ? T(acc + v[k]) : acc;
            const uint32_t step = min(uint32_t(kAccBatch), left);
            j += step;
            left -= step;
        }
        *cell = acc;
    }
}

template<typename Z>
__device__ __forceinline__ void zero_get_tile(const kargs_uag& a, const acc_tile& s)
{
    char* field = reinterpret_cast<char*>(a.ptr[s.field_slot]);
    const uint32_t ne = s.n_rows * s.levels;
    for (uint32_t e = threadIdx.x; e < ne; e += kBlock)
    {
        uint32_t r, l;
        tile_element(s, e, r, l);
        const uint32_t d = s.first_dest + r;
        const int64_t lid = a.lid64 ? ((const GHX_GLOBAL int64_t*)a.lids)[d] : ((const GHX_GLOBAL int32_t*)a.lids)[d];
        *(GHX_GLOBAL Z*)(field + lid * s.index_stride_b + int64_t(l) * s.level_stride_b) = Z(0);
    }
}

template<bool Wide>
__device__ __forceinline__ void accum_get_tiles(const kargs_uag& a)
{
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const acc_tile s = a.tiles[t];
        const bool wide = s.dtype == GHX_DT_F64 || s.dtype == GHX_DT_I64;
        if (s.zero)
        {
            if (wide) zero_get_tile<uint64_t>(a, s);
            else zero_get_tile<uint32_t>(a, s);
        }
        else if (s.dtype == GHX_DT_F32) accum_get_tile<float, Wide>(a, s);
        else if (s.dtype == GHX_DT_F64) accum_get_tile<double, Wide>(a, s);
        else if (wide) accum_get_tile<uint64_t, Wide>(a, s);
        else accum_get_tile<uint32_t, Wide>(a, s);
    }
}

__global__ __launch_bounds__(kBlock) void k_accum_get_u(kargs_uag a)
{
    if (a.rec64) accum_get_tiles<true>(a);
    else accum_get_tiles<false>(a);
}

// ---------------------------------------------------------------------------------------------
// k_accum_s: the adjoint accumulate of structured fields (saccum_plan, ghx_saccum_plan.cpp).
//
// A field's send boxes overlap, so the planner has cut their union into disjoint sub-boxes whose
// cells all have the same sources. A workgroup takes one tile of one sub-box (its record at the
// tile's index), a lane one vector of up to 16 B of a row: it loads the cell vector once, walks
// the sub-box's source records in list order — ascending (entry, box) — and stores the cell once.
// The tile and source records are the same for the whole workgroup and are read through the
// constant address space (scalar loads); what a lane issues is payload only: one load of the cell,
// one load per source, one store. The loads of kAccBatch sources are issued together, the adds
// stay in list order per element of the vector; the list's remainder (1 to 3 sources, uniform)
// loads exactly those, so a list of one — a face — takes no duplicate load. Zero tiles store zero
// vectors and load nothing from the field. 64-bit offsets, no LDS, no atomics.
// ---------------------------------------------------------------------------------------------
#define GHX_CONST __attribute__((address_space(4)))

template<typename T, int N>
struct vec_of
{
    typedef T type __attribute__((ext_vector_type(N)));
};
template<typename T>
struct vec_of<T, 1>
{
    typedef T type;
};

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return uint64_t(lo) | (uint64_t(hi) << 32); }

__device__ __forceinline__ sacc_tile load_tile_s(const GHX_CONST sacc_tile* tiles, uint32_t t)
{
    const GHX_CONST u32x4* p = (const GHX_CONST u32x4*)(tiles + t);
    u32x4 r[sizeof(sacc_tile) / 16];
#pragma unroll
    for (uint32_t k = 0; k < sizeof(sacc_tile) / 16; ++k) r[k] = p[k];
    sacc_tile s;
    __builtin_memcpy(&s, r, sizeof(sacc_tile));
    return s;
}

// the vector of source record j that lies at outer coordinates c, byte column col of a sub-box row
template<typename V>
__device__ __forceinline__ V load_src(const kargs_sa& a, const GHX_CONST sacc_src* srcs, uint32_t j,
                                      const uint32_t (&c)[4], uint32_t col, bool deep)
{
    const GHX_CONST u32x4* p = (const GHX_CONST u32x4*)(srcs + j);
    const u32x4 r0 = p[0], r1 = p[1], r2 = p[2];  // buf_off, stride[0] | stride[1], [2] | [3], slot
    const char* b = reinterpret_cast<const char*>(a.buf_ptr[r2.z]) + u64_of(r0.x, r0.y);
    uint64_t off = uint64_t(c[0]) * u64_of(r0.z, r0.w) + uint64_t(c[1]) * u64_of(r1.x, r1.y) + col;
    if (deep) off += uint64_t(c[2]) * u64_of(r1.z, r1.w) + uint64_t(c[3]) * u64_of(r2.x, r2.y);
    return *(const GHX_GLOBAL V*)(b + off);
}

// k_accum_get_s: where that vector lies, and the record's flags word. A field source (flags bit 0)
// is a receiving field's halo cells, read in place of a buffer
template<typename V>
__device__ __forceinline__ GHX_GLOBAL V* src_addr(const kargs_sa& a, const GHX_CONST sacc_src* srcs, uint32_t j,
                                                  const uint32_t (&c)[4], uint32_t col, bool deep, uint32_t& flags)
{
    const GHX_CONST u32x4* p = (const GHX_CONST u32x4*)(srcs + j);
    const u32x4 r0 = p[0], r1 = p[1], r2 = p[2];
    char* b = reinterpret_cast<char*>(a.buf_ptr[r2.z]) + u64_of(r0.x, r0.y);
    uint64_t off = uint64_t(c[0]) * u64_of(r0.z, r0.w) + uint64_t(c[1]) * u64_of(r1.x, r1.y) + col;
    if (deep) off += uint64_t(c[2]) * u64_of(r1.z, r1.w) + uint64_t(c[3]) * u64_of(r2.x, r2.y);
    flags = r2.w;
    return (GHX_GLOBAL V*)(b + off);
}

// the loads of N sources from record j on, issued together; then, in a launch with zero_halos, zero
// bytes over those that are field sources (a wave-uniform branch per source: the flags come from the
// scalar path), each by the lane that loaded it; then the adds, in list order. Signed
// (k_accum_get_x): a source whose flags carry the bit `sel` — the lane's component, one for the
// whole vector — is negated before its add: a sign-bit flip for floats, two's complement for
// integers (negate_elem's, ghx_kernels.hip), so the sum's bits are those of adding the buffer cell
// the rotating reverse pack would have stored
template<typename V, int N, bool Signed>
__device__ __forceinline__ V get_batch(const kargs_sa& a, const GHX_CONST sacc_src* srcs, uint32_t j,
                                       const uint32_t (&c)[4], uint32_t col, bool deep, V acc, uint32_t sel)
{
    GHX_GLOBAL V* p[N];
    uint32_t fl[N];
    V v[N];
#pragma unroll
    for (uint32_t k = 0; k < uint32_t(N); ++k)
    {
        p[k] = src_addr<V>(a, srcs, j + k, c, col, deep, fl[k]);
        v[k] = *p[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < uint32_t(N); ++k)
        if (a.zero_src & fl[k]) *p[k] = V(0);
#pragma unroll
    for (uint32_t k = 0; k < uint32_t(N); ++k)
    {
        if constexpr (Signed) acc = acc + ((fl[k] & sel) ? -v[k] : v[k]);
        else acc = acc + v[k];
    }
    return acc;
}

template<typename T, int W, bool Get = false, bool Signed = false>
__device__ __forceinline__ void accum_tile_s(const kargs_sa& a, const sacc_tile& s, const GHX_CONST sacc_src* srcs)
{
    typedef typename vec_of<T, W / int(sizeof(T))>::type V;
    constexpr int w = W == 16 ? 4 : W == 8 ? 3 : 2;
    char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]) + s.field_off;
    const bool deep = s.n_outer > 2;
    const uint32_t nv = sacc_vectors(s, w);
    for (uint32_t i = threadIdx.x; i < nv; i += kBlock)
    {
        uint32_t c[4], col;
        sacc_decode(s, i, w, c, col);
        int64_t foff = int64_t(c[0]) * s.stride[0] + int64_t(c[1]) * s.stride[1] + int64_t(col);
        if (deep) foff += int64_t(c[2]) * s.stride[2] + int64_t(c[3]) * s.stride[3];
        GHX_GLOBAL V* cell = (GHX_GLOBAL V*)(field + foff);
        V acc = *cell;
        uint32_t j = s.first_src, left = s.n_src;  // uniform
        if constexpr (Get)
        {
            // the flags bit of the lane's component (components 0 and 1 alone change sign); where
            // the row is the vector of components the planner has made the lanes take elements
            uint32_t sel = 0;
            if constexpr (Signed)
            {
                const uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];  // selects, no indexing
                const uint32_t ci = s.comp == kSaccCompNone  ? 0u
                                    : s.comp == kSaccCompRow ? col / uint32_t(sizeof(T))
                                    : s.comp == 1            ? c0
                                    : s.comp == 2            ? c1
                                    : s.comp == 3            ? c2
                                                             : c3;
                sel = ci < 2u ? (1u << kSaccNegShift) << ci : 0u;
            }
            for (; left >= uint32_t(kAccBatch); j += kAccBatch, left -= kAccBatch)
                acc = get_batch<V, kAccBatch, Signed>(a, srcs, j, c, col, deep, acc, sel);
            if (left == 3) acc = get_batch<V, 3, Signed>(a, srcs, j, c, col, deep, acc, sel);
            else if (left == 2) acc = get_batch<V, 2, Signed>(a, srcs, j, c, col, deep, acc, sel);
            else if (left == 1) acc = get_batch<V, 1, Signed>(a, srcs, j, c, col, deep, acc, sel);
            *cell = acc;
            continue;
        }
        while (left >= uint32_t(kAccBatch))
        {
            V v[kAccBatch];
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k) v[k] = load_src<V>(a, srcs, j + k, c, col, deep);
#pragma unroll
            for (uint32_t k = 0; k < kAccBatch; ++k) acc = acc + v[k];
            j += kAccBatch;
            left -= kAccBatch;
        }
        if (left == 3)
        {
            const V v0 = load_src<V>(a, srcs, j, c, col, deep), v1 = load_src<V>(a, srcs, j + 1, c, col, deep),
                    v2 = load_src<V>(a, srcs, j + 2, c, col, deep);
            acc = acc + v0;
            acc = acc + v1;
            acc = acc + v2;
        }
        else if (left == 2)
        {
            const V v0 = load_src<V>(a, srcs, j, c, col, deep), v1 = load_src<V>(a, srcs, j + 1, c, col, deep);
            acc = acc + v0;
            acc = acc + v1;
        }
        else if (left == 1)
            acc = acc + load_src<V>(a, srcs, j, c, col, deep);
        *cell = acc;
    }
}

template<int W>
__device__ __forceinline__ void zero_tile_s(const kargs_sa& a, const sacc_tile& s)
{
    typedef typename vec_of<uint32_t, W / 4>::type V;
    constexpr int w = W == 16 ? 4 : W == 8 ? 3 : 2;
    char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]) + s.field_off;
    const uint32_t nv = sacc_vectors(s, w);
    for (uint32_t i = threadIdx.x; i < nv; i += kBlock)
    {
        uint32_t c[4], col;
        sacc_decode(s, i, w, c, col);
        const int64_t foff = int64_t(c[0]) * s.stride[0] + int64_t(c[1]) * s.stride[1] + int64_t(c[2]) * s.stride[2] +
                             int64_t(c[3]) * s.stride[3] + int64_t(col);
        *(GHX_GLOBAL V*)(field + foff) = V(0);
    }
}

template<typename T, bool Get = false, bool Signed = false>
__device__ __forceinline__ void accum_tile_sw(const kargs_sa& a, const sacc_tile& s, const GHX_CONST sacc_src* srcs, int w)
{
    if (w == 4) accum_tile_s<T, 16, Get, Signed>(a, s, srcs);
    else if constexpr (sizeof(T) == 8) accum_tile_s<T, 8, Get, Signed>(a, s, srcs);
    else if (w == 3) accum_tile_s<T, 8, Get, Signed>(a, s, srcs);
    else accum_tile_s<T, 4, Get, Signed>(a, s, srcs);
}

template<bool Get, bool Signed = false>
__device__ __forceinline__ void accum_tiles_s(const kargs_sa& a)
{
    const GHX_CONST sacc_tile* tiles = (const GHX_CONST sacc_tile*)reinterpret_cast<uintptr_t>(a.tiles);
    const GHX_CONST sacc_src* srcs = (const GHX_CONST sacc_src*)reinterpret_cast<uintptr_t>(a.srcs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const sacc_tile s = load_tile_s(tiles, t);
        const int w = sacc_width(s, a.field_ptr[s.field_slot], a.buf_mis8, a.buf_mis16);
        if (s.zero)
        {
            if (w == 4) zero_tile_s<16>(a, s);
            else if (w == 3) zero_tile_s<8>(a, s);
            else zero_tile_s<4>(a, s);
        }
        else if (s.dtype == GHX_DT_F32) accum_tile_sw<float, Get, Signed>(a, s, srcs, w);
        else if (s.dtype == GHX_DT_F64) accum_tile_sw<double, Get, Signed>(a, s, srcs, w);
        else if (s.dtype == GHX_DT_I64) accum_tile_sw<uint64_t, Get, Signed>(a, s, srcs, w);
        else accum_tile_sw<uint32_t, Get, Signed>(a, s, srcs, w);
    }
}

__global__ __launch_bounds__(kBlock) void k_accum_s(kargs_sa a) { accum_tiles_s<false>(a); }

// k_accum_get_s: k_accum_s's walk with a source taken from the buffers or, a field source, from the
// halo cells of a receiving field of the same launch (ghx_saccum_get_create). The planner has
// verified that one (cell, source) pair reads a halo cell and that nothing else touches it, so the
// lane that loaded a halo vector may store zero bytes over it (zero_halos) with no other ordering.
__global__ __launch_bounds__(kBlock) void k_accum_get_s(kargs_sa a) { accum_tiles_s<true>(a); }

// k_accum_get_x: k_accum_get_s's walk for a cubed-sphere exchange. A self message's source is the
// halo cell whose image under the edge's transform the owner cell is: its record holds the image of
// the sub-box's origin and signed byte strides (mod 2^64, so the same unsigned products address it),
// and in its flags the vector components the edge negates. A transposed or reversed source has made
// the planner cut the rows into elements, a lane then walks the owner field in order and the halo
// across it; a vector (z- or component-fastest rows) has one component or, where the row is the
// components, one element per lane, so one sign serves a lane's whole vector. Its own instantiation:
// k_accum_s and k_accum_get_s compile as they did.
__global__ __launch_bounds__(kBlock) void k_accum_get_x(kargs_sa a) { accum_tiles_s<true, true>(a); }

// one launch of an accumulate kernel over the first a.n_tiles tiles (A: the kernel's kargs_*)
template<typename K, typename A>
int launch_acc(K kernel, const char* what, const A& a, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    grid = grid < a.n_tiles ? grid : a.n_tiles;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (t_timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
    {
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, e0, e1, 0, a);
        t_timing->emplace_back(e0, e1);
    }
    else
    {
        if (e0) (void)hipEventDestroy(e0);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, a);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
    {
        set_error(std::string(what) + " kernel launch failed: " + hipGetErrorString(err));
        return GHX_ERR_HIP;
    }
    return GHX_OK;
}
}  // namespace

int launch_accum_get_x(const kargs_sa& a, void* stream, uint32_t grid)
{
    return launch_acc(k_accum_get_x, "cubed-sphere adjoint get-accumulate", a, stream, grid);
}

int launch_accum_get_s(const kargs_sa& a, void* stream, uint32_t grid)
{
    return launch_acc(k_accum_get_s, "structured adjoint get-accumulate", a, stream, grid);
}

int launch_accum_s(const kargs_sa& a, void* stream, uint32_t grid)
{
    return launch_acc(k_accum_s, "structured adjoint accumulate", a, stream, grid);
}

int launch_accum_get_u(const kargs_uag& a, void* stream, uint32_t grid)
{
    return launch_acc(k_accum_get_u, "adjoint get-accumulate", a, stream, grid);
}

int launch_accum_u(const kargs_ua& a, void* stream, uint32_t grid)
{
    return launch_acc(k_accum_u, "adjoint accumulate", a, stream, grid);
}

}  // namespace ghx
