// ghx_cubed_sphere.cpp — the cubed-sphere grid (include/ghex/structured/cubed_sphere/): tile
// transforms, the halo generator, make_pattern with the generator's transforming intersect, and
// the planning of receive spaces that arrive in a neighbour tile's coordinates. Host only.
//
// Six tiles of c x c cells, oriented as drawn in cubed_sphere/transform.hpp:21-38. A halo that
// crosses a cube edge is generated in the neighbour's coordinates (halo_generator.hpp:160-194),
// packed there as an ordinary box, and rotated back by the receiver's unpack
// (field_descriptor.hpp:81-108, 142-167).
#include "ghx_cubed_sphere.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace ghx
{
namespace
{
// neighbour tiles in the order -x, +x, -y, +y (transform.hpp:68-76)
constexpr int kNeighbour[6][4] = {{4, 1, 5, 2}, {0, 3, 5, 2}, {0, 3, 1, 4},
                                  {2, 5, 1, 4}, {2, 5, 3, 0}, {4, 1, 3, 0}};

// own tile coordinates -> neighbour tile coordinates (transform.hpp:40-66, 82-112):
//   x' = r[0] x + r[1] y + t[0] c + o[0],   y' = r[2] x + r[3] y + t[1] c + o[1].
// The even tiles (0, 2, 4) share one row of the reference's table, the odd ones the other.
constexpr cs_transform kTransform[2][4] = {
    {{{0, -1, 1, 0}, {1, 1}, {-1, 0}},
     {{1, 0, 0, 1}, {-1, 0}, {0, 0}},
     {{1, 0, 0, 1}, {0, 1}, {0, 0}},
     {{0, 1, -1, 0}, {-1, 1}, {0, -1}}},
    {{{1, 0, 0, 1}, {1, 0}, {0, 0}},
     {{0, -1, 1, 0}, {1, -1}, {-1, 0}},
     {{0, 1, -1, 0}, {1, 1}, {0, -1}},
     {{1, 0, 0, 1}, {0, -1}, {0, 0}}}};

void check_cube(int32_t c, int32_t levels)
{
    if (c < 1 || levels < 1) throw invalid("cube: edge_size and levels must be >= 1");
    if (int64_t(c) * c * 6 > (int64_t(1) << 31) - 1)
        throw invalid("cube: edge_size too large for int32 domain ids");
}

void check_domain(int32_t c, const ghx_cs_domain& d)
{
    if (d.tile < 0 || d.tile > 5) throw invalid("cubed-sphere domain: tile must be in 0..5");
    if (d.x_first < 0 || d.x_last >= c || d.x_first > d.x_last || d.y_first < 0 || d.y_last >= c ||
        d.y_first > d.y_last)
        throw invalid("cubed-sphere domain: x/y range must lie inside the tile");
}

struct box3
{
    int32_t f[3], l[3];
    bool empty_xy() const { return f[0] > l[0] || f[1] > l[1]; }
};

box3 intersect(const box3& a, const box3& b)
{
    box3 r;
    for (int k = 0; k < 3; ++k)
    {
        r.f[k] = std::max(a.f[k], b.f[k]);
        r.l[k] = std::min(a.l[k], b.l[k]);
    }
    return r;
}
}  // namespace

const cs_transform& cs_transform_of(int tile, int n) { return kTransform[tile & 1][n]; }

int cs_neighbour_index(int tile, int other)
{
    for (int n = 0; n < 4; ++n)
        if (kNeighbour[tile][n] == other) return n;
    return -1;
}

int32_t cs_domain_id(int32_t c, const ghx_cs_domain& d)
{
    return (d.tile * c + d.y_first) * c + d.x_first;
}

// cubed_sphere::halo_generator::operator() (halo_generator.hpp:75-198)
std::vector<cs_box> cs_halo_boxes(int32_t c, int32_t levels, const ghx_cs_domain& d,
                                  const int32_t* halos)
{
    check_cube(c, levels);
    check_domain(c, d);
    for (int k = 0; k < 4; ++k)
        if (halos[k] < 0) throw invalid("cubed-sphere halo widths must be >= 0");
    const box3 dom{{d.x_first, d.y_first, 0}, {d.x_last, d.y_last, levels - 1}};
    const box3 tile{{0, 0, 0}, {c - 1, c - 1, levels - 1}};
    // the four neighbour tiles as regions of this tile's coordinate plane (:90-104)
    box3 nb[4] = {tile, tile, tile, tile};
    nb[0].f[0] -= c;
    nb[0].l[0] -= c;
    nb[1].f[0] += c;
    nb[1].l[0] += c;
    nb[2].f[1] -= c;
    nb[2].l[1] -= c;
    nb[3].f[1] += c;
    nb[3].l[1] += c;
    // bottom, left, right, top; bottom and top own the corners (:106-146). The widths are
    // applied as [0] -x, [1] +x, [2] -y, [3] +y.
    box3 reg[4] = {dom, dom, dom, dom};
    reg[0].f[0] -= halos[0];
    reg[0].f[1] -= halos[2];
    reg[0].l[0] = dom.l[0] + halos[1];
    reg[0].l[1] = dom.f[1] - 1;
    reg[1].f[0] -= halos[0];
    reg[1].l[0] = dom.f[0] - 1;
    reg[2].f[0] = dom.l[0] + 1;
    reg[2].l[0] = dom.l[0] + halos[1];
    reg[3].f[0] -= halos[0];
    reg[3].f[1] = dom.l[1] + 1;
    reg[3].l[0] = dom.l[0] + halos[1];
    reg[3].l[1] = dom.l[1] + halos[3];
    std::vector<cs_box> out;
    auto piece = [&](const box3& h, const box3& g, int32_t tile_id) {
        cs_box r{};
        for (int k = 0; k < 3; ++k)
        {
            // local = the region's local box moved with the cut (:206-214): the domain's local
            // box starts at 0, so local = global - domain first on this tile's plane
            r.b.lf[k] = h.f[k] - dom.f[k];
            r.b.ll[k] = h.l[k] - dom.f[k];
            r.b.gf[k] = g.f[k];
            r.b.gl[k] = g.l[k];
        }
        r.tile = tile_id;
        out.push_back(r);
    };
    for (const box3& h : reg)
    {
        const box3 own = intersect(h, tile);
        if (!own.empty_xy()) piece(own, own, d.tile);
        for (int n = 0; n < 4; ++n)
        {
            const box3 x = intersect(h, nb[n]);
            if (x.empty_xy()) continue;
            // re-expressed in the neighbour's coordinates, first/last swapped on reversed
            // axes (:167-192)
            const cs_transform& t = cs_transform_of(d.tile, n);
            int32_t f[2], l[2];
            t.apply(x.f[0], x.f[1], c, f);
            t.apply(x.l[0], x.l[1], c, l);
            box3 g = x;
            g.f[0] = t.reversed_x() ? l[0] : f[0];
            g.l[0] = t.reversed_x() ? f[0] : l[0];
            g.f[1] = t.reversed_y() ? l[1] : f[1];
            g.l[1] = t.reversed_y() ? f[1] : l[1];
            piece(x, g, kNeighbour[d.tile][n]);
        }
    }
    return out;
}

// make_pattern<structured::grid> (include/ghex/structured/pattern.hpp:214-329) with the
// cubed-sphere generator: every domain's halo boxes against every domain's extent through the
// seven-argument intersect (halo_generator.hpp:227-283); tags and send maps are the shared second
// half (finish_structured_pattern). A halo box and an extent on different tiles do not meet.
// (The reference returns the box reversed there, which its caller reads as empty unless the box
// is a single cell in every coordinate; that one-cell, one-level corner case is treated as
// empty here too.)
int cs_make_pattern(int32_t c, int32_t levels, const ghx_cs_domain* doms, int n,
                    const int32_t* halos, int my_rank, pattern_set& out)
{
    check_cube(c, levels);
    if (n < 1) throw invalid("cubed-sphere pattern: need at least one domain");
    std::vector<pattern_domain> pd(static_cast<size_t>(n));
    int world = 0;
    for (int a = 0; a < n; ++a)
    {
        check_domain(c, doms[a]);
        if (doms[a].rank < 0) throw invalid("cubed-sphere pattern: negative rank");
        world = std::max(world, doms[a].rank + 1);
        pd[a].id = cs_domain_id(c, doms[a]);
        pd[a].rank = doms[a].rank;
        pd[a].first[0] = doms[a].x_first;
        pd[a].first[1] = doms[a].y_first;
        pd[a].first[2] = 0;
        for (int b = 0; b < a; ++b)
            if (pd[b].id == pd[a].id) throw invalid("cubed-sphere pattern: two domains share (tile, x_first, y_first)");
    }
    std::vector<std::vector<int>> by_rank(world);
    for (int a = 0; a < n; ++a) by_rank[doms[a].rank].push_back(a);
    std::vector<recv_map> recv(static_cast<size_t>(n));
    for (int a = 0; a < n; ++a)
    {
        const ghx_cs_domain& d = doms[a];
        for (const cs_box& h : cs_halo_boxes(c, levels, d, halos))
        {
            // halos that are empty in local coordinates are dropped (pattern.hpp:260-264)
            if (h.b.lf[0] > h.b.ll[0] || h.b.lf[1] > h.b.ll[1] || h.b.lf[2] > h.b.ll[2]) continue;
            for (int j = 0; j < world; ++j)
                for (int k : by_rank[j])
                {
                    const ghx_cs_domain& o = doms[k];
                    if (o.tile != h.tile) continue;
                    const int32_t of[3] = {o.x_first, o.y_first, 0};
                    const int32_t ol[3] = {o.x_last, o.y_last, levels - 1};
                    is_pair x{};
                    bool ok = true;
                    for (int q = 0; q < 3; ++q)
                    {
                        x.gf[q] = std::max(h.b.gf[q], of[q]);
                        x.gl[q] = std::min(h.b.gl[q], ol[q]);
                        if (x.gf[q] > x.gl[q]) ok = false;
                    }
                    if (!ok) continue;
                    if (h.tile == d.tile)
                    {
                        for (int q = 0; q < 3; ++q)
                        {
                            x.lf[q] = h.b.lf[q] + (x.gf[q] - h.b.gf[q]);
                            x.ll[q] = h.b.ll[q] + (x.gl[q] - h.b.gl[q]);
                        }
                    }
                    else
                    {
                        // back through the inverse transform into this domain's local
                        // coordinates (halo_generator.hpp:241-280)
                        const cs_transform& t = cs_transform_of(d.tile, cs_neighbour_index(d.tile, h.tile));
                        int32_t p[2], q2[2];
                        t.invert(x.gf[0], x.gf[1], c, p);
                        t.invert(x.gl[0], x.gl[1], c, q2);
                        const int32_t df[2] = {d.x_first, d.y_first};
                        for (int q = 0; q < 2; ++q)
                        {
                            x.lf[q] = std::min(p[q], q2[q]) - df[q];
                            x.ll[q] = std::max(p[q], q2[q]) - df[q];
                        }
                        x.lf[2] = h.b.lf[2] + (x.gf[2] - h.b.gf[2]);
                        x.ll[2] = h.b.ll[2] + (x.gl[2] - h.b.gl[2]);
                    }
                    auto& sp = recv[a].by_id[pd[k].id];
                    sp.rank = o.rank;
                    sp.boxes.push_back(x);
                    sp.tiles.push_back(h.tile);
                }
        }
    }
    const int rc = finish_structured_pattern(3, pd, recv, my_rank, out);
    out.cs_edge = c;
    return rc;
}

// ---------------------------------------------------------------------------------------------
// planning of receive spaces
// ---------------------------------------------------------------------------------------------
void check_cs_item(const ghx_field_desc& f, const ghx_cs_item& cs)
{
    validate_field(f);
    if (f.dim - (f.has_components ? 1 : 0) != 3)
        throw invalid("a cubed-sphere field has the three spatial dimensions x, y, z");
    if (cs.edge_size < 1) throw invalid("cubed-sphere item: edge_size must be >= 1");
    if (cs.tile < 0 || cs.tile > 5) throw invalid("cubed-sphere item: tile must be in 0..5");
    if (cs.value_kind < 0 || cs.value_kind > 2) throw invalid("cubed-sphere item: value_kind must be 0, 1 or 2");
    if (cs.is_vector &&
        !((cs.value_kind == 1 || cs.value_kind == 2) && (f.elem_size == 4 || f.elem_size == 8)))
        throw invalid("a cubed-sphere vector field must hold 4- or 8-byte floats or signed "
                      "integers (value_kind 1 or 2): its components change sign across cube edges");
}

void cs_plan_space(cs_recv_plan& out, const ghx_field_desc& f, const ghx_cs_item& cs,
                   const is_pair& sp, int32_t gtile, int32_t field_slot, int32_t buf_slot,
                   uint64_t buf_off, uint64_t* space_bytes)
{
    const int D = f.dim;
    const int64_t elem = f.elem_size;
    const int64_t nc = f.num_components;
    int64_t lext[3], gext[3];
    for (int k = 0; k < 3; ++k)
    {
        lext[k] = int64_t(sp.ll[k]) - sp.lf[k] + 1;
        gext[k] = int64_t(sp.gl[k]) - sp.gf[k] + 1;
        if (lext[k] <= 0) throw invalid("iteration space: first must be <= last");
    }
    *space_bytes = uint64_t(lext[0] * lext[1] * lext[2] * nc * elem);
    ghx_box local{};
    for (int k = 0; k < 3; ++k)
    {
        local.first[k] = sp.lf[k];
        local.last[k] = sp.ll[k];
    }
    auto ordinary = [&] {
        add_box_segments(out.segs, f, local, 0, 0, buf_off);
        out.gf.resize(out.segs.size(), field_slot);
        out.gb.resize(out.segs.size(), buf_slot);
        out.sbytes += *space_bytes;
    };
    if (gtile == cs.tile)
    {
        ordinary();
        return;
    }
    const int n = cs_neighbour_index(cs.tile, gtile);
    if (n < 0) throw invalid("iteration space from a tile that is no edge neighbour of the field's tile");
    const cs_transform& t = cs_transform_of(cs.tile, n);
    if (!t.switched_xy())
    {
        // translation only: the buffer box has the local box's shape and orientation
        for (int k = 0; k < 3; ++k)
            if (gext[k] != lext[k]) throw invalid("iteration space: local and global extents differ");
        ordinary();
        return;
    }
    ++out.n_rotated;
    // The buffer cell (x', y', z, k) is field cell T^-1(x', y') - domain first (field_descriptor
    // .hpp:81-96). Both corners of the global box must map onto the local box's corners.
    const int32_t c = cs.edge_size;
    int32_t p0[2], p1[2];
    t.invert(sp.gf[0], sp.gf[1], c, p0);
    t.invert(sp.gl[0], sp.gl[1], c, p1);
    const int32_t df[2] = {cs.first_x, cs.first_y};
    for (int k = 0; k < 2; ++k)
    {
        p0[k] -= df[k];
        p1[k] -= df[k];
        if (std::min(p0[k], p1[k]) != sp.lf[k] || std::max(p0[k], p1[k]) != sp.ll[k])
            throw invalid("iteration space: the local box is not the image of the global box "
                          "under the tile transform");
    }
    if (gext[2] != lext[2]) throw invalid("iteration space: local and global level ranges differ");
    // bounds against the declared extents, as add_box_segments checks them
    for (int k = 0; k < 3; ++k)
        if (f.extents[k] > 0 && (int64_t(sp.lf[k]) + f.offsets[k] < 0 ||
                                 int64_t(sp.ll[k]) + f.offsets[k] >= f.extents[k]))
            throw invalid("iteration space outside the field extents");
    if (f.has_components && f.extents[D - 1] > 0 && nc > f.extents[D - 1])
        throw invalid("iteration space outside the field extents");
    // per buffer dim (x', y', z, component): extent and signed field byte stride. x' advances
    // the field by (r[0], r[1]) cells in (x, y), y' by (r[2], r[3]).
    const int64_t sx = f.byte_strides[0], sy = f.byte_strides[1];
    int64_t bext[GHX_MAX_DIM], bstr[GHX_MAX_DIM];
    bext[0] = gext[0];
    bstr[0] = t.r[0] * sx + t.r[1] * sy;
    bext[1] = gext[1];
    bstr[1] = t.r[2] * sx + t.r[3] * sy;
    bext[2] = gext[2];
    bstr[2] = f.byte_strides[2];
    if (f.has_components)
    {
        bext[3] = nc;
        bstr[3] = f.byte_strides[3];
    }
    const int64_t field_off = (int64_t(p0[0]) + f.offsets[0]) * sx + (int64_t(p0[1]) + f.offsets[1]) * sy +
                              (int64_t(sp.lf[2]) + f.offsets[2]) * f.byte_strides[2];
    // buffer order: the dims by layout value, fastest first (the dense box of make_buffer_desc,
    // cubed_sphere/field_descriptor.hpp:187-203)
    int by_speed[GHX_MAX_DIM];
    for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
    // vector components that change sign (field_descriptor.hpp:97-104)
    uint8_t neg = 0;
    if (cs.is_vector)
    {
        if (t.r[2] == -1) neg |= 1;
        if (t.r[1] == -1 && nc > 1) neg |= 2;
    }
    const int fast = by_speed[0];
    const bool pow2 = elem <= 16 && (elem & (elem - 1)) == 0;
    const bool moved = fast < 2 && f.byte_strides[fast] == elem;  // the stride-1 axis is x or y
    if (*space_bytes >= (uint64_t(1) << 31) - kMaxTileBytes)
        throw invalid("rotated iteration space of 2 GiB or more");
    if ((moved && pow2) || neg)
    {
        xseg b{};
        b.field_off = field_off;
        b.buf_off = buf_off;
        b.comp_axis = -1;
        for (int k = 0; k < 4; ++k)
        {
            b.ext[k] = 1;
            b.stride[k] = 0;
        }
        for (int k = 0; k < D; ++k)
        {
            b.ext[k] = uint32_t(bext[by_speed[k]]);
            b.stride[k] = bstr[by_speed[k]];
            if (f.has_components && by_speed[k] == D - 1) b.comp_axis = k;
        }
        b.elem = uint32_t(elem);
        b.neg_mask = neg;
        b.neg_kind = uint8_t(cs.value_kind);
        b.field_slot = field_slot;
        b.buf_slot = buf_slot;
        b.tile_elems = g_tune.x_tile_elems;
        out.xs.push_back(b);
        return;
    }
    // contiguous rows survive the rotation (z or the component is stride-1), or nothing is
    // contiguous anyway: an ordinary segment whose outer dims are the buffer's, with the
    // rotated (signed) field strides
    seg_s s{};
    int k0 = 0;
    if (bstr[fast] == elem)
    {
        s.row_bytes = uint32_t(bext[fast] * elem);
        k0 = 1;
    }
    else s.row_bytes = uint32_t(elem);
    int no = 0;
    for (int k = 0; k < 4; ++k)
    {
        s.ext[k] = 1;
        s.stride[k] = 0;
    }
    for (int k = k0; k < D; ++k)
    {
        if (bext[by_speed[k]] == 1) continue;
        s.ext[no] = uint32_t(bext[by_speed[k]]);
        s.stride[no] = bstr[by_speed[k]];
        ++no;
    }
    s.n_outer = uint8_t(no);
    s.field_off = field_off;
    s.buf_off = buf_off;
    s.bytes = uint32_t(*space_bytes);
    finish_segment(s);
    out.segs.push_back(s);
    out.gf.push_back(field_slot);
    out.gb.push_back(buf_slot);
    out.sbytes += *space_bytes;
}

// The receiving side of ANY space cs_plan_space has accepted, as a transformed box: per axis of
// the buffer's dense box the extent and the signed field byte stride, the field offset of buffer
// cell 0 and the components to negate. For the spaces cs_plan_space itself transforms this is
// the box it makes; own-tile and translation-only spaces have the field's own strides.
xseg cs_space_box(const ghx_field_desc& f, const ghx_cs_item& cs, const is_pair& sp, int32_t gtile,
                  int32_t field_slot, int32_t buf_slot, uint64_t buf_off)
{
    const int D = f.dim;
    const int64_t elem = f.elem_size;
    if (elem < 1 || elem > 16 || (elem & (elem - 1)))
        throw invalid("a self tile record needs an element size of 1, 2, 4, 8 or 16 bytes");
    int r[4] = {1, 0, 0, 1};
    int32_t p0[2] = {sp.lf[0], sp.lf[1]};  // the field cell of the global box's first cell
    uint8_t neg = 0;
    if (gtile != cs.tile)
    {
        const int n = cs_neighbour_index(cs.tile, gtile);
        if (n < 0) throw invalid("iteration space from a tile that is no edge neighbour of the field's tile");
        const cs_transform& t = cs_transform_of(cs.tile, n);
        if (t.switched_xy())
        {
            for (int k = 0; k < 4; ++k) r[k] = t.r[k];
            t.invert(sp.gf[0], sp.gf[1], cs.edge_size, p0);
            p0[0] -= cs.first_x;
            p0[1] -= cs.first_y;
            if (cs.is_vector)
            {
                if (t.r[2] == -1) neg |= 1;
                if (t.r[1] == -1 && f.num_components > 1) neg |= 2;
            }
        }
    }
    const int64_t sx = f.byte_strides[0], sy = f.byte_strides[1];
    int64_t bext[GHX_MAX_DIM] = {1, 1, 1, 1}, bstr[GHX_MAX_DIM] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) bext[k] = int64_t(sp.gl[k]) - sp.gf[k] + 1;
    bstr[0] = r[0] * sx + r[1] * sy;
    bstr[1] = r[2] * sx + r[3] * sy;
    bstr[2] = f.byte_strides[2];
    if (f.has_components)
    {
        bext[3] = f.num_components;
        bstr[3] = f.byte_strides[3];
    }
    int by_speed[GHX_MAX_DIM];
    for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
    xseg b{};
    b.field_off = (int64_t(p0[0]) + f.offsets[0]) * sx + (int64_t(p0[1]) + f.offsets[1]) * sy +
                  (int64_t(sp.lf[2]) + f.offsets[2]) * f.byte_strides[2];
    b.buf_off = buf_off;
    b.comp_axis = -1;
    for (int k = 0; k < 4; ++k)
    {
        b.ext[k] = 1;
        b.stride[k] = 0;
    }
    for (int k = 0; k < D; ++k)
    {
        b.ext[k] = uint32_t(bext[by_speed[k]]);
        b.stride[k] = bstr[by_speed[k]];
        if (f.has_components && by_speed[k] == D - 1) b.comp_axis = k;
    }
    b.elem = uint32_t(elem);
    b.neg_mask = neg;
    b.neg_kind = uint8_t(cs.value_kind);
    b.field_slot = field_slot;
    b.buf_slot = buf_slot;
    b.tile_elems = g_tune.x_tile_elems;
    if (b.bytes() >= (uint64_t(1) << 31) - kMaxTileBytes) throw invalid("rotated iteration space of 2 GiB or more");
    return b;
}

}  // namespace ghx
