// cs_check.hpp — what the stand-alone cubed-sphere host programs (cs_host_check, cs_self_host_check,
// cs_put_host_check) share: the CHECK macro, the fixture (domains, pattern, fields), an element
// of up to 16 bytes with its negation, bounds-checked and access-recording field accessors for
// the replays, the host model of the kernels' short-form offset, and the walk over every halo cell
// with the reference's geometry (cs_transform_of, cubed_sphere/field_descriptor.hpp:81-108) that
// the expectations are computed from. The replays themselves take their divisions, offsets, tile
// decode and negation predicate from the library's ghx_addr.hpp, the kernels' own copy.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../ghex_amd/csrc/ghx_addr.hpp"
#include "../../ghex_amd/csrc/ghx_cubed_sphere.hpp"
#include "../../ghex_amd/csrc/ghx_exchange.hpp"

namespace cs_check
{
using namespace ghx;

inline int g_fail = 0;
#define CHECK(c)                                                                 \
    do                                                                           \
    {                                                                            \
        if (!(c))                                                                \
        {                                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);              \
            if (++cs_check::g_fail > 20) std::exit(1);                           \
        }                                                                        \
    } while (0)

struct config
{
    int c, levels, halos[4], nx, ny;  // nx x ny domains per tile
};

struct spec
{
    int elem, nc, vector, kind;
};

struct field
{
    ghx_field_desc d;
    ghx_cs_item cs;
    int dom;
    spec sp;
    std::vector<unsigned char> mem, first, want;  // replayed, initial, expected
    std::vector<unsigned char> written, read;     // per byte
    // byte offset of local cell (x, y, z) component k
    int64_t offset(int x, int y, int z, int k) const
    {
        return (x + d.offsets[0]) * d.byte_strides[0] + (y + d.offsets[1]) * d.byte_strides[1] +
               z * d.byte_strides[2] + k * d.byte_strides[3];
    }
};

// a (x, y, z, k) field of one domain with `h` halo cells, memory order by `layout`
inline field make_field(const ghx_cs_domain& dom, int c, int levels, int h, const int* layout, const spec& s)
{
    field f{};
    const int shape[4] = {dom.x_last - dom.x_first + 1 + 2 * h, dom.y_last - dom.y_first + 1 + 2 * h,
                          levels, s.nc};
    f.d.dim = 4;
    f.d.elem_size = s.elem;
    int64_t stride = s.elem;
    for (int v = 3; v >= 0; --v)
        for (int d = 0; d < 4; ++d)
            if (layout[d] == v)
            {
                f.d.byte_strides[d] = stride;
                stride *= shape[d];
            }
    for (int d = 0; d < 4; ++d)
    {
        f.d.layout[d] = layout[d];
        f.d.offsets[d] = d < 2 ? h : 0;
        f.d.extents[d] = shape[d];
    }
    f.d.num_components = s.nc;
    f.d.has_components = 1;
    f.cs = {dom.tile, dom.x_first, dom.y_first, c, s.vector, s.kind};
    f.sp = s;
    f.mem.resize(size_t(stride));
    f.written.assign(size_t(stride), 0);
    f.read.assign(size_t(stride), 0);
    return f;
}

// an element of up to 16 bytes, little endian: its first `elem` bytes count
struct value
{
    uint64_t lo = 0, hi = 0;
    bool operator==(const value& o) const { return lo == o.lo && hi == o.hi; }
};

inline value truncated(value v, int elem)
{
    if (elem < 16) v.hi = 0;
    if (elem < 8) v.lo &= (uint64_t(1) << (8 * elem)) - 1;
    return v;
}

// sign-bit flip (kind 1) or two's-complement negation (kind 2) of an element of any width
inline value negated(value v, int elem, int kind)
{
    if (kind == 1)
    {
        if (elem == 16) v.hi ^= uint64_t(1) << 63;
        else v.lo ^= uint64_t(1) << (8 * elem - 1);
        return v;
    }
    value r;
    r.lo = uint64_t(0) - v.lo;
    r.hi = ~v.hi + (v.lo == 0 ? 1 : 0);
    return truncated(r, elem);
}

// field_offset_f<NDIV> of ghx_kernels.hip (device-only: its products are v_mul_u32_u24), with the
// segment's field_off added; every product's operands must be below 2^24
inline uint32_t mul24(uint32_t a, uint32_t b)
{
    CHECK(a < (1u << 24) && b < (1u << 24));
    return a * b;
}

inline int64_t offset_f(const seg_s& s, uint32_t p)
{
    const uint32_t row = fastdiv(p, s.mag_row);
    uint32_t off = p - mul24(row, s.row_bytes);
    const uint32_t q0 = fastdiv(row, s.mag_ext[0]);
    off += mul24(row - mul24(q0, s.ext[0]), uint32_t(s.stride[0]));
    if (s.amode == 1) off += mul24(q0, uint32_t(s.stride[1]));
    else
    {
        const uint32_t q1 = fastdiv(q0, s.mag_ext[1]);
        off += mul24(q0 - mul24(q1, s.ext[1]), uint32_t(s.stride[1]));
        off += mul24(q1, uint32_t(s.stride[2]));
    }
    return s.field_off + int64_t(off);
}

// The fixture: nx x ny domains on each of the six tiles, all on rank 0, their pattern, and one
// field per spec and domain (field set by field set, each over all domains) of pseudo-random bytes.
struct fixture
{
    config cfg;
    std::vector<ghx_cs_domain> doms;
    ghx_pattern* pat = nullptr;
    std::vector<field> fields;

    fixture(const config& c, const int* layout, const std::vector<spec>& specs) : cfg(c)
    {
        const int sx = cfg.c / cfg.nx, sy = cfg.c / cfg.ny;
        for (int t = 0; t < 6; ++t)
            for (int j = 0; j < cfg.ny; ++j)
                for (int i = 0; i < cfg.nx; ++i)
                    doms.push_back({0, t, i * sx, (i + 1) * sx - 1, j * sy, (j + 1) * sy - 1});
        CHECK(ghx_cs_pattern_create(cfg.c, cfg.levels, doms.data(), int(doms.size()), cfg.halos, 0,
                                    &pat) == GHX_OK);
        if (!pat) return;
        int h = 1;
        for (int k = 0; k < 4; ++k) h = std::max(h, cfg.halos[k]);
        for (const spec& s : specs)
            for (size_t a = 0; a < doms.size(); ++a)
            {
                fields.push_back(make_field(doms[a], cfg.c, cfg.levels, h, layout, s));
                field& f = fields.back();
                f.dom = int(a);
                uint64_t x = 0x9E3779B97F4A7C15ull * (fields.size() + 1);
                for (unsigned char& b : f.mem)
                {
                    x = x * 6364136223846793005ull + 1442695040888963407ull;
                    b = static_cast<unsigned char>(x >> 56);
                }
                f.first = f.mem;
                f.want = f.mem;
            }
    }
    fixture(const fixture&) = delete;
    ~fixture()
    {
        if (pat) ghx_pattern_destroy(pat);
    }

    // the exchange items of the fields, in field order (one pattern, align = the element size)
    void items(std::vector<ghx_exchange_item>& it, std::vector<ghx_cs_item>& cs) const
    {
        for (const field& f : fields)
        {
            ghx_exchange_item i{};
            i.pattern = pat;
            i.local_index = int32_t(f.dom);
            i.kind = 0;
            i.field = f.d;
            i.align = f.sp.elem;
            it.push_back(i);
            cs.push_back(f.cs);
        }
    }

    // Bounds-checked accesses of a replay. Reads are recorded per byte. Writes are recorded and
    // kept aside until apply(): a launch's workgroups (and the other ranks' launches of the same
    // epoch) run in no order, so a read must never see a write — check_accesses() below.
    bool in_field(int slot, int64_t off, size_t n) const
    {
        return slot >= 0 && size_t(slot) < fields.size() && off >= 0 &&
               size_t(off) + n <= fields[size_t(slot)].mem.size();
    }
    bool src_read(int slot, int64_t off, void* to, size_t n)
    {
        const bool ok = in_field(slot, off, n);
        CHECK(ok);
        if (!ok) return false;
        std::memcpy(to, fields[size_t(slot)].mem.data() + off, n);
        for (size_t i = 0; i < n; ++i) fields[size_t(slot)].read[size_t(off) + i] = 1;
        return true;
    }
    void dst_write(int slot, int64_t off, const void* from, size_t n)
    {
        const bool ok = in_field(slot, off, n);
        CHECK(ok);
        if (!ok) return;
        dwrites.push_back({slot, off, pending.size(), n});
        pending.insert(pending.end(), static_cast<const unsigned char*>(from),
                       static_cast<const unsigned char*>(from) + n);
        for (size_t i = 0; i < n; ++i) ++fields[size_t(slot)].written[size_t(off) + i];
    }
    void apply()
    {
        for (const dwrite& w : dwrites)
            std::memcpy(fields[size_t(w.slot)].mem.data() + w.off, pending.data() + w.at, w.n);
        dwrites.clear();
        pending.clear();
    }
    // every field is as expected; no byte is written twice or both read and written; returns the
    // bytes written
    uint64_t check_accesses() const
    {
        uint64_t halo_bytes = 0;
        for (const field& f : fields)
        {
            CHECK(f.mem == f.want);
            for (size_t i = 0; i < f.mem.size(); ++i)
            {
                CHECK(f.written[i] <= 1);
                CHECK(!(f.written[i] && f.read[i]));  // no byte the launch reads is one it writes
                halo_bytes += f.written[i];
            }
        }
        return halo_bytes;
    }

private:
    struct dwrite
    {
        int slot;
        int64_t off;
        size_t at, n;  // the bytes: pending[at, at + n)
    };
    std::vector<dwrite> dwrites;
    std::vector<unsigned char> pending;
};

// the dense box of a space in a field's layout order (regular/field_descriptor.hpp:114-129):
// byte stride per (x, y, z, k) and the box's bytes
struct dense_box
{
    int64_t ext[4], bstride[4], bytes;
    dense_box(const field& f, const int32_t* first, const int32_t* last)
    {
        for (int d = 0; d < 3; ++d) ext[d] = last[d] - first[d] + 1;
        ext[3] = f.sp.nc;
        int order[4];
        for (int d = 0; d < 4; ++d) order[3 - f.d.layout[d]] = d;  // fastest first
        bytes = f.sp.elem;
        for (int k = 0; k < 4; ++k)
        {
            bstride[order[k]] = bytes;
            bytes *= ext[order[k]];
        }
    }
    // byte position of box coordinates bc (checked to lie inside)
    int64_t at(const int64_t (&bc)[4]) const
    {
        int64_t loc = 0;
        for (int q = 0; q < 4; ++q)
        {
            CHECK(bc[q] >= 0 && bc[q] < ext[q]);
            loc += bc[q] * bstride[q];
        }
        return loc;
    }
};

// One halo cell of a receive space as the reference's unpack sees it: local cell (x, y, z)
// component k of field f, the sender's global coordinates g of that cell under the tile
// transform, and whether the component is negated.
struct halo_cell
{
    int x, y, z, k;
    int32_t g[2];
    bool neg;
};

// Walks every cell of every receive space of every field. begin(f, entry, box index) is called
// once per space and returns whether to walk it; cell(f, entry, box index, halo_cell) once per
// cell. Returns the number of cells walked. The geometry is the reference's, not the planner's.
template<typename Begin, typename Cell>
uint64_t for_each_halo_cell(fixture& fx, Begin&& begin, Cell&& cell)
{
    uint64_t cells = 0;
    for (field& f : fx.fields)
    {
        const ghx_cs_domain& dom = fx.doms[size_t(f.dom)];
        for (const halo_entry& e : fx.pat->doms[size_t(f.dom)].recv)
            for (size_t i = 0; i < e.boxes.size(); ++i)
            {
                if (!begin(f, e, i)) continue;
                const is_pair& bx = e.boxes[i];
                const int n = e.tiles[i] == dom.tile ? -1 : cs_neighbour_index(dom.tile, e.tiles[i]);
                halo_cell h{};
                for (h.x = bx.lf[0]; h.x <= bx.ll[0]; ++h.x)
                    for (h.y = bx.lf[1]; h.y <= bx.ll[1]; ++h.y)
                        for (h.z = bx.lf[2]; h.z <= bx.ll[2]; ++h.z)
                            for (h.k = 0; h.k < f.sp.nc; ++h.k)
                            {
                                h.g[0] = h.x + dom.x_first;
                                h.g[1] = h.y + dom.y_first;
                                h.neg = false;
                                if (n >= 0)
                                {
                                    const cs_transform& t = cs_transform_of(dom.tile, n);
                                    t.apply(h.x + dom.x_first, h.y + dom.y_first, fx.cfg.c, h.g);
                                    h.neg = f.sp.vector &&
                                            ((h.k == 0 && t.r[2] == -1) || (h.k == 1 && t.r[1] == -1));
                                }
                                cell(f, e, i, h);
                                ++cells;
                            }
            }
    }
    return cells;
}

// The replay of one transformed tile record as the kernels' walk indexes it (ghx_addr.hpp):
// elem(c, to) is called with the tile coordinates and the destination field offset of every
// element inside the tile. Checks the tile's size and that its elements fill its byte count.
template<typename Elem>
void replay_tile(const seg_x& s, int x_tile_elems, Elem&& elem)
{
    const uint32_t total = s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3];
    CHECK(total <= uint32_t(x_tile_elems ? x_tile_elems : 256));
    uint32_t stored = 0;
    for (uint32_t i = 0; i < total; ++i)
    {
        uint32_t c[4];
        const bool inside = tile_decode(s, i, c);
        CHECK(c[3] < s.tdim[3]);
        if (!inside) continue;
        if (elem(c, affine_offset(s.field_off, s.stride, c))) ++stored;
    }
    CHECK(uint64_t(stored) << s.elog2 == s.bytes);
}

// the element as the walk stores it to the receiving field
inline value stored_value(const seg_x& s, const uint32_t (&c)[4], value v)
{
    return tile_negates(s, c) ? negated(v, 1 << s.elog2, s.neg_kind) : v;
}
}  // namespace cs_check
