// cs_host_check — stand-alone host program (its own main; links the library's sources) that
// runs the cubed-sphere fixture geometries through ghx_cs_pattern_create and the device-less
// planning of ghx_cs_exchange_create, then replays every planned unpack segment and every
// transformed tile record on the host, exactly as k_copy / k_unpack_x index them, with every
// buffer and field access bounds-checked, and compares each halo cell with the buffer element
// the reference's unpack reads for it (cubed_sphere/field_descriptor.hpp:81-108). Elements of
// 1, 2, 4, 8 and 16 bytes, both negations (sign-bit flip, two's complement) at 4 and 8 bytes, each
// at the default tile size and at x_tile_elems 32, 48 and 4096. Built with
// -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../ghex_amd/csrc/ghx_cubed_sphere.hpp"
#include "../../ghex_amd/csrc/ghx_exchange.hpp"

using namespace ghx;

namespace
{
int g_fail = 0;
#define CHECK(c)                                                                 \
    do                                                                           \
    {                                                                            \
        if (!(c))                                                                \
        {                                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);              \
            if (++g_fail > 20) std::exit(1);                                     \
        }                                                                        \
    } while (0)

struct config
{
    int c, levels, halos[4], nx, ny;  // nx x ny domains per tile
};

uint32_t fdiv(uint32_t n, magic_u32 m)
{
    const uint32_t t = uint32_t((uint64_t(m.m) * n) >> 32);
    return (t + ((n - t) >> m.s1)) >> m.s2;
}

struct field
{
    ghx_field_desc d;
    ghx_cs_item cs;
    std::vector<unsigned char> mem;
};

// a (x, y, z, k) field of one domain with `h` halo cells, memory order by `layout`
field make_field(const ghx_cs_domain& dom, int c, int levels, int h, const int* layout, int elem,
                 int nc, int vector, int kind)
{
    field f{};
    const int shape[4] = {dom.x_last - dom.x_first + 1 + 2 * h, dom.y_last - dom.y_first + 1 + 2 * h,
                          levels, nc};
    f.d.dim = 4;
    f.d.elem_size = elem;
    int64_t stride = elem;
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
    f.d.num_components = nc;
    f.d.has_components = 1;
    f.cs = {dom.tile, dom.x_first, dom.y_first, c, vector, kind};
    f.mem.assign(size_t(stride), 0xC3);
    return f;
}

// an element of up to 16 bytes, little endian: its first `elem` bytes count
struct value
{
    uint64_t lo = 0, hi = 0;
    bool operator==(const value& o) const { return lo == o.lo && hi == o.hi; }
};

value truncated(value v, int elem)
{
    if (elem < 16) v.hi = 0;
    if (elem < 8) v.lo &= (uint64_t(1) << (8 * elem)) - 1;
    return v;
}

// element id stored in the receive buffers: (buffer index << 24) ^ element index, truncated to
// the element size (4 and 8 bytes); 1- and 2-byte elements hold high bits of its product with an
// odd constant instead (the id's own low bits would repeat every 256 elements along a row), and
// a 16-byte element holds that product in its upper half
value elem_id(size_t buffer, uint64_t index, int elem)
{
    value v;
    v.lo = (uint64_t(buffer + 1) << 24) ^ index;
    const uint64_t mixed = v.lo * 0x9E3779B97F4A7C15ull;
    if (elem < 4) v.lo = mixed >> 40;
    v.hi = mixed | 1;
    return truncated(v, elem);
}

// sign-bit flip (kind 1) or two's-complement negation (kind 2) of an element of any width
value negated(value v, int elem, int kind)
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

void run(const config& cfg, const int* layout, int elem, int nc, int vector, int kind,
         int x_tile_elems)
{
    // a planning knob: read when the exchange is created
    if (x_tile_elems) CHECK(ghx_tune("x_tile_elems", x_tile_elems) == GHX_OK);
    std::vector<ghx_cs_domain> doms;
    const int sx = cfg.c / cfg.nx, sy = cfg.c / cfg.ny;
    for (int t = 0; t < 6; ++t)
        for (int j = 0; j < cfg.ny; ++j)
            for (int i = 0; i < cfg.nx; ++i)
                doms.push_back({0, t, i * sx, (i + 1) * sx - 1, j * sy, (j + 1) * sy - 1});
    ghx_pattern* pat = nullptr;
    CHECK(ghx_cs_pattern_create(cfg.c, cfg.levels, doms.data(), int(doms.size()), cfg.halos, 0,
                                &pat) == GHX_OK);
    if (!pat) return;
    int h = 1;
    for (int k = 0; k < 4; ++k) h = std::max(h, cfg.halos[k]);
    std::vector<field> fields;
    std::vector<ghx_exchange_item> items;
    std::vector<ghx_cs_item> cs;
    for (size_t a = 0; a < doms.size(); ++a)
    {
        fields.push_back(make_field(doms[a], cfg.c, cfg.levels, h, layout, elem, nc, vector, kind));
        ghx_exchange_item it{};
        it.pattern = pat;
        it.local_index = int32_t(a);
        it.kind = 0;
        it.field = fields.back().d;
        it.align = elem;
        items.push_back(it);
        cs.push_back(fields.back().cs);
    }
    ghx_exchange* ex = nullptr;
    const int rc = ghx_cs_exchange_create(items.data(), cs.data(), int(items.size()), &ex);
    if (x_tile_elems) CHECK(ghx_tune("reset", 0) == GHX_OK);
    if (rc != GHX_OK) std::printf("create: %s\n", ghx_last_error());
    CHECK(rc == GHX_OK);
    if (!ex)
    {
        ghx_pattern_destroy(pat);
        return;
    }
    // receive buffers filled with element ids
    std::vector<std::vector<unsigned char>> bufs;
    for (size_t b = 0; b < ex->recv.size(); ++b)
    {
        bufs.emplace_back(size_t(ex->recv[b].size));
        CHECK(ex->recv[b].size % uint64_t(elem) == 0);
        for (uint64_t i = 0; i < ex->recv[b].size / uint64_t(elem); ++i)
        {
            const value v = elem_id(b, i, elem);
            std::memcpy(bufs[b].data() + i * elem, &v, size_t(elem));
        }
    }
    auto field_write = [&](int slot, int64_t off, const unsigned char* src, size_t n) {
        CHECK(slot >= 0 && size_t(slot) < fields.size());
        CHECK(off >= 0 && size_t(off) + n <= fields[size_t(slot)].mem.size());
        if (off >= 0 && size_t(off) + n <= fields[size_t(slot)].mem.size())
            std::memcpy(fields[size_t(slot)].mem.data() + off, src, n);
    };
    // ordinary segments, row by row as field_offset_s decodes them (general form)
    auto replay_s = [&](const std::vector<seg_s>& segs, const std::vector<int32_t>& fm,
                        const std::vector<int32_t>& bm) {
        for (const seg_s& s : segs)
        {
            const int fs = fm.empty() ? s.field_slot : fm[s.field_slot];
            const int bs = bm.empty() ? s.buf_slot : bm[s.buf_slot];
            const uint32_t rows = s.bytes / s.row_bytes;
            CHECK(s.buf_off + s.bytes <= bufs[size_t(bs)].size());
            for (uint32_t r = 0; r < rows; ++r)
            {
                uint32_t q = r;
                int64_t off = s.field_off;
                for (int k = 0; k < 4; ++k)
                {
                    const uint32_t ck = k < 3 ? q % s.ext[k] : q;
                    if (k < 3) q /= s.ext[k];
                    off += int64_t(ck) * s.stride[k];
                }
                field_write(fs, off, bufs[size_t(bs)].data() + s.buf_off + uint64_t(r) * s.row_bytes,
                            s.row_bytes);
            }
        }
    };
    if (ex->sunpack)
    {
        replay_s(ex->sunpack->host_segs, ex->sunpack->fmap, ex->sunpack->bmap);
        for (const auto& g : ex->sunpack->more) replay_s(g->host_segs, g->fmap, g->bmap);
    }
    // transformed tile records, as k_unpack_x walks them: field order, transposed buffer reads
    if (ex->xunpack)
        for (const auto& g : ex->xunpack->groups)
            for (const seg_x& s : g->host)
            {
                const int fs = g->fmap.empty() ? s.field_slot : g->fmap[s.field_slot];
                const int bs = g->bmap.empty() ? s.buf_slot : g->bmap[s.buf_slot];
                const uint32_t total = s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3];
                CHECK(total <= 4096);
                CHECK(total <= uint32_t(x_tile_elems ? x_tile_elems : 256));
                CHECK((1 << s.elog2) == elem);
                uint32_t stored = 0;
                for (uint32_t i = 0; i < total; ++i)
                {
                    const uint32_t q0 = fdiv(i, s.mag[0]), c0 = i - q0 * s.tdim[0];
                    const uint32_t q1 = fdiv(q0, s.mag[1]), c1 = q0 - q1 * s.tdim[1];
                    const uint32_t c3 = fdiv(q1, s.mag[2]), c2 = q1 - c3 * s.tdim[2];
                    CHECK(c3 < s.tdim[3]);
                    if (c0 >= s.act[0] || c1 >= s.act[1] || c2 >= s.act[2] || c3 >= s.act[3]) continue;
                    const uint32_t cc[4] = {c0, c1, c2, c3};
                    uint64_t bi = 0;
                    int64_t off = s.field_off;
                    for (int k = 0; k < 4; ++k)
                    {
                        bi += uint64_t(cc[k]) * s.bstride[k];
                        off += int64_t(cc[k]) * s.stride[k];
                    }
                    const uint64_t from = s.buf_off + (bi << s.elog2);
                    const bool inside = from + (uint64_t(1) << s.elog2) <= bufs[size_t(bs)].size();
                    CHECK(inside);
                    if (!inside) continue;
                    value v;
                    std::memcpy(&v, bufs[size_t(bs)].data() + from, size_t(1) << s.elog2);
                    const uint32_t comp = s.comp0 + (s.comp_pos < 4 ? cc[s.comp_pos] : 0);
                    if (comp < 2 && ((s.neg_mask >> comp) & 1)) v = negated(v, 1 << s.elog2, s.neg_kind);
                    field_write(fs, off, reinterpret_cast<const unsigned char*>(&v), size_t(1) << s.elog2);
                    ++stored;
                }
                CHECK(uint64_t(stored) << s.elog2 == s.bytes);
            }
    // expectation: communication_object::allocate's buffer layout (fields in item order, aligned)
    // and the reference's buffer() for every cell of every receive space
    std::map<std::pair<int32_t, int32_t>, uint64_t> fill;
    uint64_t cells = 0;
    for (size_t a = 0; a < doms.size(); ++a)
    {
        const field& f = fields[a];
        const domain_pattern& dp = pat->doms[a];
        int order[4];
        for (int d = 0; d < 4; ++d) order[3 - f.d.layout[d]] = d;  // fastest first
        for (const halo_entry& e : dp.recv)
        {
            size_t b = 0;
            while (b < ex->recv.size() &&
                   !(ex->recv[b].first_id == dp.id && ex->recv[b].second_id == e.key.remote_id))
                ++b;
            CHECK(b < ex->recv.size());
            if (b >= ex->recv.size()) continue;
            uint64_t& at = fill[{dp.id, e.key.remote_id}];
            at = (at + uint64_t(elem) - 1) / uint64_t(elem) * uint64_t(elem);
            for (size_t i = 0; i < e.boxes.size(); ++i)
            {
                const is_pair& sp = e.boxes[i];
                const int n = e.tiles[i] == doms[a].tile ? -1 : cs_neighbour_index(doms[a].tile, e.tiles[i]);
                int64_t ext[4] = {sp.gl[0] - sp.gf[0] + 1, sp.gl[1] - sp.gf[1] + 1,
                                  sp.gl[2] - sp.gf[2] + 1, nc};
                int64_t bstride[4], acc = elem;
                for (int k = 0; k < 4; ++k)
                {
                    bstride[order[k]] = acc;
                    acc *= ext[order[k]];
                }
                for (int x = sp.lf[0]; x <= sp.ll[0]; ++x)
                    for (int y = sp.lf[1]; y <= sp.ll[1]; ++y)
                        for (int z = sp.lf[2]; z <= sp.ll[2]; ++z)
                            for (int k = 0; k < nc; ++k)
                            {
                                int32_t g[2] = {x + doms[a].x_first, y + doms[a].y_first};
                                bool neg = false;
                                if (n >= 0)
                                {
                                    const cs_transform& t = cs_transform_of(doms[a].tile, n);
                                    t.apply(x + doms[a].x_first, y + doms[a].y_first, cfg.c, g);
                                    neg = vector && ((k == 0 && t.r[2] == -1) || (k == 1 && t.r[1] == -1));
                                }
                                const int64_t bc[4] = {g[0] - sp.gf[0], g[1] - sp.gf[1], z - sp.gf[2], k};
                                int64_t loc = 0;
                                for (int q = 0; q < 4; ++q)
                                {
                                    CHECK(bc[q] >= 0 && bc[q] < ext[q]);
                                    loc += bc[q] * bstride[q];
                                }
                                value want = elem_id(b, (at + uint64_t(loc)) / uint64_t(elem), elem);
                                if (neg) want = negated(want, elem, f.cs.value_kind);
                                const int64_t off = (x + f.d.offsets[0]) * f.d.byte_strides[0] +
                                                    (y + f.d.offsets[1]) * f.d.byte_strides[1] +
                                                    z * f.d.byte_strides[2] + k * f.d.byte_strides[3];
                                value got;
                                std::memcpy(&got, f.mem.data() + off, size_t(elem));
                                CHECK(got == want);
                                ++cells;
                            }
                at += uint64_t(acc);
            }
        }
    }
    for (size_t b = 0; b < ex->recv.size(); ++b)
        CHECK((fill[{ex->recv[b].first_id, ex->recv[b].second_id}] == ex->recv[b].size));
    int32_t nrec = 0, ntiles = 0, nrot = 0;
    uint64_t xbytes = 0;
    CHECK(ghx_cs_plan_info(ex, &nrec, &xbytes, &ntiles, &nrot) == GHX_OK);
    std::printf("c=%d levels=%d layout=%d%d%d%d elem=%d nc=%d vector=%d kind=%d x_tile_elems=%d: "
                "%llu halo cells, %d rotated spaces, %d transformed records in %d tiles\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], elem, nc, vector, kind,
                x_tile_elems ? x_tile_elems : 256, static_cast<unsigned long long>(cells), nrot,
                nrec, ntiles);
    // every record is covered, by no fewer tiles than its elements need
    CHECK(uint64_t(ntiles) * uint64_t(x_tile_elems ? x_tile_elems : 256) * uint64_t(elem) >= xbytes);
    CHECK(ntiles >= nrec);
    ghx_exchange_destroy(ex);
    ghx_pattern_destroy(pat);
}
}  // namespace

int main()
{
    const config cfgs[] = {{10, 3, {2, 2, 2, 2}, 2, 2}, {6, 2, {1, 2, 0, 3}, 1, 1},
                           {70, 5, {3, 3, 3, 3}, 1, 1}, {8, 2, {2, 2, 2, 2}, 2, 1}};
    const int layouts[][4] = {{3, 2, 1, 0}, {2, 3, 1, 0}, {1, 2, 3, 0}, {0, 1, 2, 3}};
    for (const config& cfg : cfgs)
        for (const auto& layout : layouts)
            for (const int tile : {0, 32, 48, 4096})  // 0: the default, no knob set
            {
                run(cfg, layout, 8, 1, 0, 1, tile);
                run(cfg, layout, 4, 3, 1, 2, tile);
                run(cfg, layout, 8, 2, 1, 1, tile);
                // the other widths (scalars: opaque bits), and each width's other negation
                run(cfg, layout, 1, 1, 0, 0, tile);
                run(cfg, layout, 2, 3, 0, 0, tile);
                run(cfg, layout, 16, 1, 0, 0, tile);
                run(cfg, layout, 8, 3, 1, 2, tile);
                run(cfg, layout, 4, 2, 1, 1, tile);
            }
    std::printf(g_fail ? "cs_host_check: %d FAILURES\n" : "cs_host_check: OK\n", g_fail);
    return g_fail ? 1 : 0;
}
