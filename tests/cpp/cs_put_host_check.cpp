// cs_put_host_check — stand-alone host program (its own main; links the library's sources) for
// the cubed-sphere put. It plans the cubed-sphere fixture geometries (ghx_cs_pattern_create,
// no device), pairs every send halo with the receive halo of the same domain pair as the bulk
// object does, builds ONE put plan over all messages with ghx_cs_put_create, and replays every
// pair record and every put tile record (seg_xs) on the host, with the kernels' own address
// arithmetic (ghx_addr.hpp) exactly as k_put_cs indexes them, with every source and destination
// access bounds-checked. The fields it leaves are compared, whole, with the reference's
// semantics read straight from the senders' fields: pack = the sender's box in its own
// coordinates (regular/field_descriptor.hpp:114-150), unpack = the rotating, negating read of
// cubed_sphere/field_descriptor.hpp:81-108. It also checks that every halo byte is written exactly
// once and that no byte the launch reads is a byte it writes. Elements of 1 to 16 bytes, both
// negations at 4 and 8 bytes, two fields of different width in one plan, each at the default
// tile size and at x_tile_elems 32, 48 and 4096. Built with -fsanitize=address,undefined by
// tools/cs_host_sanitize.sh; needs no GPU.
#include "cs_check.hpp"

using namespace cs_check;

namespace
{
void run(const config& cfg, const int* layout, const std::vector<spec>& specs, int x_tile_elems)
{
    fixture fx(cfg, layout, specs);
    if (!fx.pat) return;
    ghx_pattern* pat = fx.pat;
    const std::vector<ghx_cs_domain>& doms = fx.doms;
    std::vector<field>& fields = fx.fields;  // field slot = index, on both sides
    std::map<int32_t, int> dom_of_id;
    for (size_t a = 0; a < doms.size(); ++a) dom_of_id[pat->doms[a].id] = int(a);
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
            const int64_t fo = field_offset_s(s, p), uo = field_offset_s(q, p);
            if (s.amode) CHECK(offset_f(s, p) == fo);
            if (q.amode) CHECK(offset_f(q, p) == uo);
            if (p % w == 0) CHECK(fo % w == 0 && uo % w == 0);
            unsigned char v = 0;
            if (!fx.src_read(s.field_slot, fo, &v, 1)) continue;
            fx.dst_write(q.field_slot, uo, &v, 1);
        }
        pair_bytes += end - start;
    }

    // ------------------------------------------------------------------ put tile records
    uint64_t x_bytes = 0;
    for (const seg_xs& r : pp.x_recs)
    {
        const seg_x& s = r.x;
        const size_t e = size_t(1) << s.elog2;
        CHECK(int(e) == fields[r.src_slot].sp.elem && int(e) == fields[s.field_slot].sp.elem);
        replay_tile(s, x_tile_elems, [&](const uint32_t (&c)[4], int64_t to) {
            value v;
            if (!fx.src_read(r.src_slot, affine_offset(r.src_off, r.src_stride, c), &v, e)) return false;
            v = stored_value(s, c, v);
            fx.dst_write(s.field_slot, to, &v, e);
            return true;
        });
        x_bytes += s.bytes;
    }
    fx.apply();

    // ------------------------------------------------------------------ the reference
    // halo cell (x, y, z, k) of a receive space = the sender's cell at the transformed global
    // coordinates, components negated where the neighbour's axes point the other way
    uint64_t payload = 0;
    const uint64_t cells = for_each_halo_cell(
        fx,
        [&](field& f, const halo_entry& e, size_t i) {
            CHECK(e.tiles[i] == doms[size_t(dom_of_id.at(e.key.remote_id))].tile);
            (void)f;
            return true;
        },
        [&](field& f, const halo_entry& e, size_t i, const halo_cell& h) {
            const is_pair& bx = e.boxes[i];
            const int sd = dom_of_id.at(e.key.remote_id);
            const field& sf = fields[size_t(&f - fields.data()) - size_t(f.dom) + size_t(sd)];
            const ghx_cs_domain& sdom = doms[size_t(sd)];
            CHECK(h.g[0] >= bx.gf[0] && h.g[0] <= bx.gl[0] && h.g[1] >= bx.gf[1] && h.g[1] <= bx.gl[1]);
            // the sender's own cell: inside its domain, never its halo
            const int sxl = h.g[0] - sdom.x_first, syl = h.g[1] - sdom.y_first;
            CHECK(sxl >= 0 && h.g[0] <= sdom.x_last && syl >= 0 && h.g[1] <= sdom.y_last);
            value v;
            std::memcpy(&v, sf.first.data() + sf.offset(sxl, syl, h.z, h.k), size_t(f.sp.elem));
            if (h.neg) v = negated(v, f.sp.elem, f.sp.kind);
            std::memcpy(f.want.data() + f.offset(h.x, h.y, h.z, h.k), &v, size_t(f.sp.elem));
            payload += uint64_t(f.sp.elem);
        });
    // ------------------------------------------------------------------ comparison
    CHECK(pair_bytes + x_bytes == payload);
    CHECK(plan_bytes == payload);
    CHECK(fx.check_accesses() == payload);
    std::printf("c=%d levels=%d layout=%d%d%d%d fields=%zu (elem %d..) x_tile_elems=%d: %llu halo "
                "cells in %zu messages, %d pair tiles, %d put tile records in %d tiles\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], specs.size(),
                specs[0].elem, x_tile_elems ? x_tile_elems : 256,
                static_cast<unsigned long long>(cells), src.size(), npair, nxrec, nxtiles);
    ghx_put_destroy(put);
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
