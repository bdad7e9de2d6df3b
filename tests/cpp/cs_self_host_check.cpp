// cs_self_host_check — stand-alone host program (its own main; links the library's sources) for
// the fused cubed-sphere self exchange. It plans the cubed-sphere fixture geometries with all
// domains on one rank (ghx_cs_pattern_create, ghx_cs_exchange_create, no device), then replays
// every pair record and every self tile record (seg_xs) of the fused plan on the host, with the
// kernels' own address arithmetic (ghx_addr.hpp) exactly as k_self_cs indexes them, with every
// source, buffer and destination access bounds-checked. The send buffers and the fields it leaves
// are compared, whole, with the reference's semantics:
// pack = the sender's dense box in its layout order (regular/field_descriptor.hpp:114-150),
// unpack = the rotating, negating read of cubed_sphere/field_descriptor.hpp:81-108. It also
// checks that every payload byte of every buffer and every halo byte is written exactly once and
// that no byte the launch reads is a byte it writes. Elements of 1 to 16 bytes, both negations
// at 4 and 8 bytes, two fields of different width in one exchange, each at the default tile size
// and at x_tile_elems 32, 48 and 4096. Built with -fsanitize=address,undefined by
// tools/cs_host_sanitize.sh; needs no GPU.
#include "cs_check.hpp"

using namespace cs_check;

namespace
{
void run(const config& cfg, const int* layout, const std::vector<spec>& specs, int x_tile_elems)
{
    fixture fx(cfg, layout, specs);
    if (!fx.pat) return;
    std::vector<field>& fields = fx.fields;
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
    int32_t fusable = 0, npair = 0, nxrec = 0, nxtiles = 0;
    CHECK(ghx_cs_self_info(ex, &fusable, &npair, &nxrec, &nxtiles) == GHX_OK);
    if (!fusable) std::printf("not fusable: %s\n", ghx_last_error());
    CHECK(fusable == 1);
    int32_t plain = 1;
    CHECK(ghx_exchange_self_fusable(ex, &plain) == GHX_OK);
    int32_t nrot = 0;
    CHECK(ghx_cs_plan_info(ex, nullptr, nullptr, nullptr, &nrot) == GHX_OK);
    CHECK(nrot == 0 || plain == 0);
    if (!fusable || !ex->cs_self)
    {
        ghx_exchange_destroy(ex);
        return;
    }
    const cs_self_plan& sp = *ex->cs_self;
    CHECK(sp.n_pair_tiles() == uint32_t(npair) && sp.n_x_tiles() == uint32_t(nxtiles));
    CHECK(ex->send.size() == ex->recv.size());

    // buffers: got (what the replay writes) and want (the reference's pack), same filler
    std::vector<std::vector<unsigned char>> got, want, bwritten;
    for (size_t b = 0; b < ex->send.size(); ++b)
    {
        got.emplace_back(size_t(ex->send[b].size), static_cast<unsigned char>(0x5A));
        want.emplace_back(size_t(ex->send[b].size), static_cast<unsigned char>(0x5A));
        bwritten.emplace_back(size_t(ex->send[b].size), static_cast<unsigned char>(0));
    }
    auto buf_write = [&](int slot, uint64_t off, const void* from, size_t n) {
        const bool ok = slot >= 0 && size_t(slot) < got.size() && off + n <= got[size_t(slot)].size();
        CHECK(ok);
        if (!ok) return;
        std::memcpy(got[size_t(slot)].data() + off, from, n);
        for (size_t i = 0; i < n; ++i) ++bwritten[size_t(slot)][size_t(off) + i];
    };

    // ------------------------------------------------------------------ pair records (k_self's)
    uint64_t pair_bytes = 0;
    for (uint32_t t = 0; t < sp.n_pair_tiles(); ++t)
    {
        const seg_s& s = sp.pair_recs[2 * t];
        const seg_s& q = sp.pair_recs[2 * t + 1];
        CHECK(s.buf_slot == q.buf_slot && s.buf_off == q.buf_off && s.bytes == q.bytes &&
              s.row_bytes == q.row_bytes && q.bytes > 0);
        CHECK(s.tile_bytes > 0 && uint64_t(s.first_tile) * s.tile_bytes < s.bytes);
        const uint32_t start = s.first_tile * s.tile_bytes;
        const uint32_t end = std::min(start + s.tile_bytes, s.bytes);
        // the vector width the kernel may choose divides rows, offsets and strides
        CHECK(s.row_bytes % (1u << s.wlog2) == 0 && q.row_bytes % (1u << q.wlog2) == 0);
        for (uint32_t p = start; p < end; ++p)
        {
            const int64_t fo = field_offset_s(s, p), uo = field_offset_s(q, p);
            if (s.amode) CHECK(offset_f(s, p) == fo);
            if (q.amode) CHECK(offset_f(q, p) == uo);
            unsigned char v = 0;
            if (!fx.src_read(s.field_slot, fo, &v, 1)) continue;
            buf_write(s.buf_slot, s.buf_off + p, &v, 1);
            fx.dst_write(q.field_slot, uo, &v, 1);
        }
        pair_bytes += end - start;
    }

    // ------------------------------------------------------------------ self tile records
    uint64_t x_bytes = 0;
    for (const seg_xs& r : sp.x_recs)
    {
        const seg_x& s = r.x;
        const size_t e = size_t(1) << s.elog2;
        replay_tile(s, x_tile_elems, [&](const uint32_t (&c)[4], int64_t to) {
            value v;
            if (!fx.src_read(r.src_slot, affine_offset(r.src_off, r.src_stride, c), &v, e)) return false;
            buf_write(s.buf_slot, s.buf_off + (uint64_t(tile_cell(s, c)) << s.elog2), &v, e);
            v = stored_value(s, c, v);
            fx.dst_write(s.field_slot, to, &v, e);
            return true;
        });
        x_bytes += s.bytes;
    }
    fx.apply();

    // ------------------------------------------------------------------ the reference: pack
    // communication_object::allocate's layout: per domain pair the fields in item order, each
    // aligned; a field's spaces back to back, each the dense box in layout order
    auto buffer_of = [&](int32_t first, int32_t second) {
        size_t b = 0;
        while (b < ex->send.size() && !(ex->send[b].first_id == first && ex->send[b].second_id == second)) ++b;
        CHECK(b < ex->send.size());
        return b;
    };
    std::map<std::pair<int32_t, int32_t>, uint64_t> fill;
    uint64_t payload = 0;
    for (field& f : fields)
    {
        const domain_pattern& dp = fx.pat->doms[size_t(f.dom)];
        const int elem = f.sp.elem, nc = f.sp.nc;
        for (const halo_entry& e : dp.send)
        {
            const size_t b = buffer_of(e.key.remote_id, dp.id);
            if (b >= ex->send.size()) continue;
            uint64_t& at = fill[{e.key.remote_id, dp.id}];
            at = (at + uint64_t(elem) - 1) / uint64_t(elem) * uint64_t(elem);
            for (const is_pair& bx : e.boxes)
            {
                const dense_box box(f, bx.lf, bx.ll);
                CHECK(at + uint64_t(box.bytes) <= want[b].size());
                if (at + uint64_t(box.bytes) > want[b].size()) continue;
                for (int x = bx.lf[0]; x <= bx.ll[0]; ++x)
                    for (int y = bx.lf[1]; y <= bx.ll[1]; ++y)
                        for (int z = bx.lf[2]; z <= bx.ll[2]; ++z)
                            for (int k = 0; k < nc; ++k)
                            {
                                const int64_t loc = box.at({x - bx.lf[0], y - bx.lf[1], z - bx.lf[2], k});
                                // `first` is the field's initial state
                                std::memcpy(want[b].data() + at + uint64_t(loc),
                                            f.first.data() + f.offset(x, y, z, k), size_t(elem));
                            }
                at += uint64_t(box.bytes);
                payload += uint64_t(box.bytes);
            }
        }
    }
    // ------------------------------------------------------------------ the reference: unpack
    fill.clear();
    size_t b = 0;      // of the space being walked: its buffer,
    uint64_t base = 0; // its first byte there
    const uint64_t cells = for_each_halo_cell(
        fx,
        [&](field& f, const halo_entry& e, size_t i) {
            const int32_t id = fx.pat->doms[size_t(f.dom)].id;
            b = buffer_of(id, e.key.remote_id);
            if (b >= ex->send.size()) return false;
            uint64_t& at = fill[{id, e.key.remote_id}];
            const uint64_t elem = uint64_t(f.sp.elem);
            base = at = (at + elem - 1) / elem * elem;
            const dense_box box(f, e.boxes[i].gf, e.boxes[i].gl);
            CHECK(base + uint64_t(box.bytes) <= want[b].size());
            if (base + uint64_t(box.bytes) > want[b].size()) return false;
            at += uint64_t(box.bytes);
            return true;
        },
        [&](field& f, const halo_entry& e, size_t i, const halo_cell& h) {
            const is_pair& bx = e.boxes[i];
            const dense_box box(f, bx.gf, bx.gl);
            const int64_t loc = box.at({h.g[0] - bx.gf[0], h.g[1] - bx.gf[1], h.z - bx.gf[2], h.k});
            value v;
            std::memcpy(&v, want[b].data() + base + uint64_t(loc), size_t(f.sp.elem));
            if (h.neg) v = negated(v, f.sp.elem, f.sp.kind);
            std::memcpy(f.want.data() + f.offset(h.x, h.y, h.z, h.k), &v, size_t(f.sp.elem));
        });
    // ------------------------------------------------------------------ comparison
    CHECK(pair_bytes + x_bytes == payload);
    for (size_t k = 0; k < got.size(); ++k)
    {
        CHECK(got[k] == want[k]);
        uint64_t more = 0;
        for (unsigned char w : bwritten[k]) more += w > 1;
        CHECK(more == 0);
    }
    CHECK(fx.check_accesses() == payload);
    std::printf("c=%d levels=%d layout=%d%d%d%d fields=%zu (elem %d..) x_tile_elems=%d: %llu halo "
                "cells, %d rotated spaces, %d pair tiles, %d self records in %d tiles\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], specs.size(),
                specs[0].elem, x_tile_elems ? x_tile_elems : 256,
                static_cast<unsigned long long>(cells), nrot, npair, nxrec, nxtiles);
    CHECK(nxtiles >= nxrec);
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
                // an fp64 scalar and an f32 3-vector in one exchange (two widths per buffer)
                run(cfg, layout, {{8, 1, 0, 1}, {4, 3, 1, 1}}, tile);
                run(cfg, layout, {{4, 3, 1, 2}}, tile);
                run(cfg, layout, {{8, 2, 1, 1}, {8, 3, 1, 2}}, tile);
                // the other widths (scalars: opaque bits)
                run(cfg, layout, {{1, 1, 0, 0}, {2, 3, 0, 0}}, tile);
                run(cfg, layout, {{16, 1, 0, 0}}, tile);
            }
    std::printf(g_fail ? "cs_self_host_check: %d FAILURES\n" : "cs_self_host_check: OK\n", g_fail);
    return g_fail ? 1 : 0;
}
