// ghx_cubed_sphere.hpp — cubed-sphere tile transforms and the planning of rotated receive spaces.
#pragma once

#include <cstdint>
#include <vector>

#include "ghx_pattern.hpp"
#include "ghx_plan.hpp"

namespace ghx
{
// cubed_sphere::transform (transform.hpp:40-66): own tile coordinates -> a neighbour's.
struct cs_transform
{
    int r[4];  // m_rotation
    int t[2];  // m_translation (in units of the edge size)
    int o[2];  // m_offset
    constexpr bool switched_xy() const { return r[0] == 0; }
    constexpr bool reversed_x() const { return switched_xy() ? r[1] == -1 : r[0] == -1; }
    constexpr bool reversed_y() const { return switched_xy() ? r[2] == -1 : r[3] == -1; }
    void apply(int32_t x, int32_t y, int32_t c, int32_t (&out)[2]) const
    {
        out[0] = r[0] * x + r[1] * y + t[0] * c + o[0];
        out[1] = r[2] * x + r[3] * y + t[1] * c + o[1];
    }
    // the inverse (the rotation part is orthogonal: its inverse is its transpose); equals the
    // reference's inverse_transform_lu entry (transform.hpp:115-128)
    void invert(int32_t xn, int32_t yn, int32_t c, int32_t (&out)[2]) const
    {
        const int32_t u = xn - t[0] * c - o[0], v = yn - t[1] * c - o[1];
        out[0] = r[0] * u + r[2] * v;
        out[1] = r[1] * u + r[3] * v;
    }
};

// transform_lu[tile][n] and the index n (-x, +x, -y, +y) of `other` among tile's neighbours (-1)
const cs_transform& cs_transform_of(int tile, int n);
int cs_neighbour_index(int tile, int other);
int32_t cs_domain_id(int32_t c, const ghx_cs_domain& d);

// The unpack side of a cubed-sphere exchange: ordinary segments (own-tile and translation-only
// spaces, rotated spaces that keep contiguous rows) with their caller slots, and the boxes of
// the transformed launch.
struct cs_recv_plan
{
    std::vector<seg_s> segs;
    std::vector<int32_t> gf, gb;
    uint64_t sbytes = 0;
    std::vector<xseg> xs;
    int32_t n_rotated = 0;
};

// refuses fields the cubed-sphere unpack cannot serve (GHX_ERR_INVALID through `invalid`)
void check_cs_item(const ghx_field_desc& f, const ghx_cs_item& cs);
// One receive space of field `f` at buf_off: appended to out.segs or out.xs. gtile = the tile of
// the space's global box. *space_bytes = its buffer bytes.
void cs_plan_space(cs_recv_plan& out, const ghx_field_desc& f, const ghx_cs_item& cs,
                   const is_pair& sp, int32_t gtile, int32_t field_slot, int32_t buf_slot,
                   uint64_t buf_off, uint64_t* space_bytes);
// The receiving side of a space cs_plan_space has accepted, as a transformed box whatever form
// cs_plan_space gave it (the fused self exchange's tile records; element sizes 1..16, powers of 2)
xseg cs_space_box(const ghx_field_desc& f, const ghx_cs_item& cs, const is_pair& sp, int32_t gtile,
                  int32_t field_slot, int32_t buf_slot, uint64_t buf_off);
}  // namespace ghx
