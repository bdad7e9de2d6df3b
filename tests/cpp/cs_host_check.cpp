// cs_host_check — stand-alone host program (its own main; links the library's sources) that
// runs the cubed-sphere fixture geometries through ghx_cs_pattern_create and the device-less
// planning of ghx_cs_exchange_create, then replays every planned unpack segment and every
// transformed tile record on the host, with the kernels' own address arithmetic (ghx_addr.hpp)
// exactly as k_copy / k_unpack_x index them, with every buffer and field access bounds-checked,
// and compares each halo cell with the buffer element the reference's unpack reads for it
// (cubed_sphere/field_descriptor.hpp:81-108). Elements of 1, 2, 4, 8 and 16 bytes, both negations
// (sign-bit flip, two's complement) at 4 and 8 bytes, each at the default tile size and at
// x_tile_elems 32, 48 and 4096. Built with -fsanitize=address,undefined by
// tools/cs_host_sanitize.sh; needs no GPU.
#include "cs_check.hpp"

using namespace cs_check;

namespace
{
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

void run(const config& cfg, const int* layout, int elem, int nc, int vector, int kind,
         int x_tile_elems)
{
    fixture fx(cfg, layout, {{elem, nc, vector, kind}});
    if (!fx.pat) return;
    for (field& f : fx.fields) f.mem.assign(f.mem.size(), 0xC3);
    std::vector<ghx_exchange_item> items;
    std::vector<ghx_cs_item> cs;
    fx.items(items, cs);
    // a planning knob: read when the exchange is created
    if (x_tile_elems) CHECK(ghx_tune("x_tile_elems", x_tile_elems) == GHX_OK);
    ghx_exchange* ex = nullptr;
    const int rc = ghx_cs_exchange_create(items.data(), cs.data(), int(items.size()), &ex);
    if (x_tile_elems) CHECK(ghx_tune("reset", 0) == GHX_OK);
    if (rc != GHX_OK) std::printf("create: %s\n", ghx_last_error());
    CHECK(rc == GHX_OK);
    if (!ex) return;
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
    // ordinary segments, row by row in the order field_offset_s decodes them
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
                CHECK(off == field_offset_s(s, r * s.row_bytes));
                fx.dst_write(fs, off, bufs[size_t(bs)].data() + s.buf_off + uint64_t(r) * s.row_bytes,
                             s.row_bytes);
            }
        }
    };
    if (ex->sunpack)
        for (const auto& g : ex->sunpack->groups) replay_s(g.host_segs, g.fmap, g.bmap);
    // transformed tile records, as k_unpack_x walks them: field order, transposed buffer reads
    if (ex->xunpack)
        for (const auto& g : ex->xunpack->groups)
            for (const seg_x& s : g.host_segs)
            {
                const int fs = g.fmap.empty() ? s.field_slot : g.fmap[s.field_slot];
                const int bs = g.bmap.empty() ? s.buf_slot : g.bmap[s.buf_slot];
                CHECK(s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3] <= 4096);
                CHECK((1 << s.elog2) == elem);
                replay_tile(s, x_tile_elems, [&](const uint32_t (&c)[4], int64_t off) {
                    const uint64_t from = s.buf_off + (uint64_t(tile_cell(s, c)) << s.elog2);
                    const bool inside = from + (uint64_t(1) << s.elog2) <= bufs[size_t(bs)].size();
                    CHECK(inside);
                    if (!inside) return false;
                    value v;
                    std::memcpy(&v, bufs[size_t(bs)].data() + from, size_t(1) << s.elog2);
                    v = stored_value(s, c, v);
                    fx.dst_write(fs, off, &v, size_t(1) << s.elog2);
                    return true;
                });
            }
    fx.apply();
    // expectation: communication_object::allocate's buffer layout (fields in item order, aligned)
    // and the reference's buffer() for every cell of every receive space
    std::map<std::pair<int32_t, int32_t>, uint64_t> fill;
    size_t b = 0;       // of the space being walked: its buffer,
    uint64_t base = 0;  // its first byte there
    const uint64_t cells = for_each_halo_cell(
        fx,
        [&](field& f, const halo_entry& e, size_t i) {
            const int32_t id = fx.pat->doms[size_t(f.dom)].id;
            b = 0;
            while (b < ex->recv.size() &&
                   !(ex->recv[b].first_id == id && ex->recv[b].second_id == e.key.remote_id))
                ++b;
            CHECK(b < ex->recv.size());
            if (b >= ex->recv.size()) return false;
            uint64_t& at = fill[{id, e.key.remote_id}];
            base = at = (at + uint64_t(elem) - 1) / uint64_t(elem) * uint64_t(elem);
            at += uint64_t(dense_box(f, e.boxes[i].gf, e.boxes[i].gl).bytes);
            return true;
        },
        [&](field& f, const halo_entry& e, size_t i, const halo_cell& h) {
            const is_pair& sp = e.boxes[i];
            const dense_box box(f, sp.gf, sp.gl);
            const int64_t loc = box.at({h.g[0] - sp.gf[0], h.g[1] - sp.gf[1], h.z - sp.gf[2], h.k});
            value want = elem_id(b, (base + uint64_t(loc)) / uint64_t(elem), elem);
            if (h.neg) want = negated(want, elem, f.cs.value_kind);
            value got;
            std::memcpy(&got, f.mem.data() + f.offset(h.x, h.y, h.z, h.k), size_t(elem));
            CHECK(got == want);
        });
    for (size_t k = 0; k < ex->recv.size(); ++k)
        CHECK((fill[{ex->recv[k].first_id, ex->recv[k].second_id}] == ex->recv[k].size));
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
