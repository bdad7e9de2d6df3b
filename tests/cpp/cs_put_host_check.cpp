// cs_put_host_check — stand-alone host program (its own main; links the library's sources) for
// the cubed-sphere put. It plans the cubed-sphere fixture geometries (ghx_cs_pattern_create,
// no device), pairs every send halo with the receive halo of the same domain pair as the bulk
// object does, builds ONE put plan over all messages with ghx_cs_put_create, and replays every
// pair record and every put tile record (seg_xs) on the host, exactly as k_put_cs indexes them,
// with every source and destination access bounds-checked. The fields it leaves are compared,
// whole, with the reference's semantics read straight from the senders' fields: pack = the
// sender's box in its own coordinates (regular/field_descriptor.hpp:114-150), unpack = the
// rotating, negating read of cubed_sphere/field_descriptor.hpp:81-108. It also checks that every
// halo byte is written exactly once and that no byte the launch reads is a byte it writes.
// Elements of 1 to 16 bytes, both negations at 4 and 8 bytes, two fields of different width in
// one plan, each at the default tile size and at x_tile_elems 32, 48 and 4096. Built with
// -fsanitize=address,undefined by tools/cs_put_host_sanitize.sh; needs no GPU.
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

struct spec
{
    int elem, nc, vector, kind;
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
    int dom;
    spec sp;
    std::vector<unsigned char> mem, first, want;  // replayed, initial, expected
    std::vector<unsigned char> written, read;     // per byte
};

// a (x, y, z, k) field of one domain with `h` halo cells, memory order by `layout`
field make_field(const ghx_cs_domain& dom, int c, int levels, int h, const int* layout, const spec& s)
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
};

value truncated(value v, int elem)
{
    if (elem < 16) v.hi = 0;
    if (elem < 8) v.lo &= (uint64_t(1) << (8 * elem)) - 1;
    return v;
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

// field_offset_s of ghx_kernels.hip
int64_t offset_s(const seg_s& s, uint32_t p)
{
    const uint32_t row = fdiv(p, s.mag_row);
    const uint32_t col = p - row * s.row_bytes;
    const uint32_t q0 = fdiv(row, s.mag_ext[0]);
    const uint32_t c0 = row - q0 * s.ext[0];
    const uint32_t q1 = fdiv(q0, s.mag_ext[1]);
    const uint32_t c1 = q0 - q1 * s.ext[1];
    const uint32_t q2 = fdiv(q1, s.mag_ext[2]);
    const uint32_t c2 = q1 - q2 * s.ext[2];
    return s.field_off + int64_t(c0) * s.stride[0] + int64_t(c1) * s.stride[1] +
           int64_t(c2) * s.stride[2] + int64_t(q2) * s.stride[3] + int64_t(col);
}

// field_offset_f<NDIV> of ghx_kernels.hip, relative to field_off; every product's operands must
// be below 2^24 (v_mul_u32_u24)
uint32_t mul24(uint32_t a, uint32_t b)
{
    CHECK(a < (1u << 24) && b < (1u << 24));
    return a * b;
}

int64_t offset_f(const seg_s& s, uint32_t p)
{
    const uint32_t row = fdiv(p, s.mag_row);
    uint32_t off = p - mul24(row, s.row_bytes);
    const uint32_t q0 = fdiv(row, s.mag_ext[0]);
    off += mul24(row - mul24(q0, s.ext[0]), uint32_t(s.stride[0]));
    if (s.amode == 1) off += mul24(q0, uint32_t(s.stride[1]));
    else
    {
        const uint32_t q1 = fdiv(q0, s.mag_ext[1]);
        off += mul24(q0 - mul24(q1, s.ext[1]), uint32_t(s.stride[1]));
        off += mul24(q1, uint32_t(s.stride[2]));
    }
    return s.field_off + int64_t(off);
}

void run(const config& cfg, const int* layout, const std::vector<spec>& specs, int x_tile_elems)
{
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
    std::map<int32_t, int> dom_of_id;
    for (size_t a = 0; a < doms.size(); ++a) dom_of_id[pat->doms[a].id] = int(a);
    // fields: field set by field set, each over all domains; field slot = index, on both sides
    std::vector<field> fields;
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
    CHECK(fields.size() < size_t(GHX_MAX_SLOTS));
    // messages: per field, each send halo with the receive halo of the same domain pair and tag
    // on the same field set's field of the receiving domain; message m is virtual buffer m
    std::vector<ghx_pack_entry> src, dst;
    std::vector<ghx_cs_item> dcs;
    std::vector<std::vector<ghx_box>> store;  // boxes of src[m], dst[m], global of dst[m]
    std::vector<std::vector<int32_t>> tstore;
    store.reserve(fields.size() * 64 * 3);
    tstore.reserve(fields.size() * 64);
    for (size_t fi = 0; fi < fields.size(); ++fi)
    {
        const field& f = fields[fi];
        const domain_pattern& dp = pat->doms[size_t(f.dom)];
        for (const halo_entry& e : dp.send)
        {
            const int rd = dom_of_id.at(e.key.remote_id);
            const size_t ti = fi - size_t(f.dom) + size_t(rd);  // same field set, receiving domain
            const halo_entry* re = nullptr;
            for (const halo_entry& r : pat->doms[size_t(rd)].recv)
                if (r.key.remote_id == dp.id && r.key.tag == e.key.tag) re = &r;
            CHECK(re != nullptr);
            if (!re) continue;
            CHECK(re->boxes.size() == e.boxes.size() && re->tiles.size() == re->boxes.size());
            const int32_t m = int32_t(src.size());
            std::vector<ghx_box> sb, db, gb;
            for (const is_pair& b : e.boxes)
            {
                ghx_box x{};
                for (int d = 0; d < 3; ++d)
                {
                    x.first[d] = b.lf[d];
                    x.last[d] = b.ll[d];
                }
                sb.push_back(x);
            }
            for (const is_pair& b : re->boxes)
            {
                ghx_box x{}, g{};
                for (int d = 0; d < 3; ++d)
                {
                    x.first[d] = b.lf[d];
                    x.last[d] = b.ll[d];
                    g.first[d] = b.gf[d];
                    g.last[d] = b.gl[d];
                }
                db.push_back(x);
                gb.push_back(g);
            }
            store.push_back(sb);
            const ghx_box* sp = store.back().data();
            store.push_back(db);
            const ghx_box* dp_ = store.back().data();
            store.push_back(gb);
            tstore.push_back(re->tiles);
            ghx_pack_entry se{}, de{};
            se.field = f.d;
            se.field_slot = int32_t(fi);
            se.buffer_slot = m;
            se.boxes = sp;
            se.n_boxes = int32_t(sb.size());
            de.field = fields[ti].d;
            de.field_slot = int32_t(ti);
            de.buffer_slot = m;
            de.boxes = dp_;
            de.n_boxes = int32_t(db.size());
            src.push_back(se);
            dst.push_back(de);
            dcs.push_back(fields[ti].cs);
        }
    }
    std::vector<const ghx_box*> gptr;
    std::vector<const int32_t*> tptr;
    for (size_t m = 0; m < dst.size(); ++m)
    {
        gptr.push_back(store[3 * m + 2].data());
        tptr.push_back(tstore[m].data());
    }
    // a planning knob: read when the plan is created
    if (x_tile_elems) CHECK(ghx_tune("x_tile_elems", x_tile_elems) == GHX_OK);
    ghx_put* put = nullptr;
    const int rc = ghx_cs_put_create(src.data(), int32_t(src.size()), dst.data(), int32_t(dst.size()),
                                     dcs.data(), gptr.data(), tptr.data(), &put);
    if (x_tile_elems) CHECK(ghx_tune("reset", 0) == GHX_OK);
    if (rc != GHX_OK) std::printf("create: %s\n", ghx_last_error());
    CHECK(rc == GHX_OK);
    if (!put || !put->cs)
    {
        CHECK(put && put->cs);
        ghx_pattern_destroy(pat);
        return;
    }
    const cs_put_plan& pp = *put->cs;
    int32_t npair = 0, nxrec = 0, nxtiles = 0, ntiles = 0;
    uint64_t plan_bytes = 0;
    CHECK(ghx_cs_put_info(put, &npair, &nxrec, &nxtiles) == GHX_OK);
    CHECK(ghx_put_info(put, &plan_bytes, &ntiles) == GHX_OK);
    CHECK(pp.n_pair_tiles() == uint32_t(npair) && pp.n_x_tiles() == uint32_t(nxtiles));
    CHECK(ntiles == npair + nxtiles && nxtiles >= nxrec);
    CHECK(pp.max_src_slot < int(fields.size()) && pp.max_dst_slot < int(fields.size()));

    // ------------------------------------------------------------------ the replay's accessors
    auto src_read = [&](int slot, int64_t off, unsigned char* to, size_t n) {
        const bool ok = slot >= 0 && size_t(slot) < fields.size() && off >= 0 &&
                        size_t(off) + n <= fields[size_t(slot)].mem.size();
        CHECK(ok);
        if (!ok) return false;
        std::memcpy(to, fields[size_t(slot)].mem.data() + off, n);
        for (size_t i = 0; i < n; ++i) fields[size_t(slot)].read[size_t(off) + i] = 1;
        return true;
    };
    // the destination writes are kept aside and applied at the end: the launch's workgroups (and
    // the other ranks' launches of the same epoch) run in no order, so a read must never see a
    // write (checked below through the read/written maps)
    struct dwrite
    {
        int slot;
        int64_t off;
        unsigned char b[16];
        size_t n;
    };
    std::vector<dwrite> dwrites;
    auto dst_write = [&](int slot, int64_t off, const unsigned char* from, size_t n) {
        const bool ok = slot >= 0 && size_t(slot) < fields.size() && off >= 0 &&
                        size_t(off) + n <= fields[size_t(slot)].mem.size();
        CHECK(ok);
        if (!ok) return;
        dwrite w{slot, off, {}, n};
        std::memcpy(w.b, from, n);
        dwrites.push_back(w);
        for (size_t i = 0; i < n; ++i) ++fields[size_t(slot)].written[size_t(off) + i];
    };

    // ------------------------------------------------------------------ pair records (k_put's)
    uint64_t pair_bytes = 0;
    for (uint32_t t = 0; t < pp.n_pair_tiles(); ++t)
    {
        const seg_s& s = pp.pair_recs[2 * t];
        const seg_s& q = pp.pair_recs[2 * t + 1];
        CHECK(s.bytes == q.bytes && s.row_bytes == q.row_bytes && q.bytes > 0);
        CHECK(s.tile_bytes > 0 && uint64_t(s.first_tile) * s.tile_bytes < s.bytes);
        const uint32_t start = s.first_tile * s.tile_bytes;
        const uint32_t end = std::min(start + s.tile_bytes, s.bytes);
        // the vector width the kernel may choose (the smaller of the two sides', narrowed by the
        // pointers) divides rows, offsets and strides of both sides
        const uint32_t w = 1u << std::min(s.wlog2, q.wlog2);
        CHECK(s.row_bytes % w == 0 && start % w == 0);
        CHECK(fields[s.field_slot].sp.elem == fields[q.field_slot].sp.elem);
        for (uint32_t p = start; p < end; ++p)
        {
            const int64_t fo = offset_s(s, p), uo = offset_s(q, p);
            if (s.amode) CHECK(offset_f(s, p) == fo);
            if (q.amode) CHECK(offset_f(q, p) == uo);
            if (p % w == 0) CHECK(fo % w == 0 && uo % w == 0);
            unsigned char v = 0;
            if (!src_read(s.field_slot, fo, &v, 1)) continue;
            dst_write(q.field_slot, uo, &v, 1);
        }
        pair_bytes += end - start;
    }

    // ------------------------------------------------------------------ put tile records
    uint64_t x_bytes = 0;
    for (const seg_xs& r : pp.x_recs)
    {
        const seg_x& s = r.x;
        const uint32_t total = s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3];
        CHECK(total <= uint32_t(x_tile_elems ? x_tile_elems : 256));
        const size_t e = size_t(1) << s.elog2;
        CHECK(int(e) == fields[r.src_slot].sp.elem && int(e) == fields[s.field_slot].sp.elem);
        uint32_t stored = 0;
        for (uint32_t i = 0; i < total; ++i)
        {
            const uint32_t q0 = fdiv(i, s.mag[0]), c0 = i - q0 * s.tdim[0];
            const uint32_t q1 = fdiv(q0, s.mag[1]), c1 = q0 - q1 * s.tdim[1];
            const uint32_t c3 = fdiv(q1, s.mag[2]), c2 = q1 - c3 * s.tdim[2];
            CHECK(c3 < s.tdim[3]);
            if (c0 >= s.act[0] || c1 >= s.act[1] || c2 >= s.act[2] || c3 >= s.act[3]) continue;
            const uint32_t cc[4] = {c0, c1, c2, c3};
            int64_t from = r.src_off, to = s.field_off;
            for (int k = 0; k < 4; ++k)
            {
                from += int64_t(cc[k]) * r.src_stride[k];
                to += int64_t(cc[k]) * s.stride[k];
            }
            value v;
            if (!src_read(r.src_slot, from, reinterpret_cast<unsigned char*>(&v), e)) continue;
            const uint32_t comp = s.comp0 + (s.comp_pos < 4 ? cc[s.comp_pos] : 0);
            if (comp < 2 && ((s.neg_mask >> comp) & 1)) v = negated(v, int(e), s.neg_kind);
            dst_write(s.field_slot, to, reinterpret_cast<unsigned char*>(&v), e);
            ++stored;
        }
        CHECK(uint64_t(stored) << s.elog2 == s.bytes);
        x_bytes += s.bytes;
    }
    for (const dwrite& w : dwrites) std::memcpy(fields[size_t(w.slot)].mem.data() + w.off, w.b, w.n);

    // ------------------------------------------------------------------ the reference
    // halo cell (x, y, z, k) of a receive space = the sender's cell at the transformed global
    // coordinates, components negated where the neighbour's axes point the other way
    uint64_t cells = 0, payload = 0;
    for (size_t fi = 0; fi < fields.size(); ++fi)
    {
        field& f = fields[fi];
        const ghx_cs_domain& dom = doms[size_t(f.dom)];
        const domain_pattern& dp = pat->doms[size_t(f.dom)];
        const int elem = f.sp.elem, nc = f.sp.nc;
        for (const halo_entry& e : dp.recv)
        {
            const int sd = dom_of_id.at(e.key.remote_id);
            const field& sf = fields[fi - size_t(f.dom) + size_t(sd)];
            const ghx_cs_domain& sdom = doms[size_t(sd)];
            for (size_t i = 0; i < e.boxes.size(); ++i)
            {
                const is_pair& bx = e.boxes[i];
                CHECK(e.tiles[i] == sdom.tile);
                const int n = e.tiles[i] == dom.tile ? -1 : cs_neighbour_index(dom.tile, e.tiles[i]);
                for (int x = bx.lf[0]; x <= bx.ll[0]; ++x)
                    for (int y = bx.lf[1]; y <= bx.ll[1]; ++y)
                        for (int z = bx.lf[2]; z <= bx.ll[2]; ++z)
                            for (int k = 0; k < nc; ++k)
                            {
                                int32_t g[2] = {x + dom.x_first, y + dom.y_first};
                                bool neg = false;
                                if (n >= 0)
                                {
                                    const cs_transform& t = cs_transform_of(dom.tile, n);
                                    t.apply(x + dom.x_first, y + dom.y_first, cfg.c, g);
                                    neg = f.sp.vector && ((k == 0 && t.r[2] == -1) || (k == 1 && t.r[1] == -1));
                                }
                                CHECK(g[0] >= bx.gf[0] && g[0] <= bx.gl[0] && g[1] >= bx.gf[1] && g[1] <= bx.gl[1]);
                                // the sender's own cell: inside its domain, never its halo
                                const int sxl = g[0] - sdom.x_first, syl = g[1] - sdom.y_first;
                                CHECK(sxl >= 0 && g[0] <= sdom.x_last && syl >= 0 && g[1] <= sdom.y_last);
                                const int64_t so = (sxl + sf.d.offsets[0]) * sf.d.byte_strides[0] +
                                                   (syl + sf.d.offsets[1]) * sf.d.byte_strides[1] +
                                                   z * sf.d.byte_strides[2] + k * sf.d.byte_strides[3];
                                value v;
                                std::memcpy(&v, sf.first.data() + so, size_t(elem));
                                if (neg) v = negated(v, elem, f.sp.kind);
                                const int64_t off = (x + f.d.offsets[0]) * f.d.byte_strides[0] +
                                                    (y + f.d.offsets[1]) * f.d.byte_strides[1] +
                                                    z * f.d.byte_strides[2] + k * f.d.byte_strides[3];
                                std::memcpy(f.want.data() + off, &v, size_t(elem));
                                ++cells;
                                payload += uint64_t(elem);
                            }
            }
        }
    }
    // ------------------------------------------------------------------ comparison
    CHECK(pair_bytes + x_bytes == payload);
    CHECK(plan_bytes == payload);
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
    CHECK(halo_bytes == payload);
    std::printf("c=%d levels=%d layout=%d%d%d%d fields=%zu (elem %d..) x_tile_elems=%d: %llu halo "
                "cells in %zu messages, %d pair tiles, %d put tile records in %d tiles\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], specs.size(),
                specs[0].elem, x_tile_elems ? x_tile_elems : 256,
                static_cast<unsigned long long>(cells), src.size(), npair, nxrec, nxtiles);
    ghx_put_destroy(put);
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
                // an fp64 scalar and an f32 3-vector in one plan (two widths)
                run(cfg, layout, {{8, 1, 0, 1}, {4, 3, 1, 1}}, tile);
                run(cfg, layout, {{4, 3, 1, 2}}, tile);
                run(cfg, layout, {{8, 2, 1, 1}, {8, 3, 1, 2}}, tile);
                // the other widths (scalars: opaque bits)
                run(cfg, layout, {{1, 1, 0, 0}, {2, 3, 0, 0}}, tile);
                run(cfg, layout, {{16, 1, 0, 0}}, tile);
            }
    std::printf(g_fail ? "cs_put_host_check: %d FAILURES\n" : "cs_put_host_check: OK\n", g_fail);
    return g_fail ? 1 : 0;
}
