// saccum_host_check — stand-alone host program (its own main; links the library's sources) for the
// structured adjoint accumulate plan: ghx_saccum_create / _info / _box / _source / _destroy, created
// without a device. The plan of one periodic 3^3 domain with halo 2 (source lists of 7, 11, 17 and
// 26) in several layouts and a plan over all 64 field and buffer slots are replayed on host arrays
// from their TILE and SOURCE records — the records a launch reads, through the kernel's own decode
// (ghx_addr.hpp) at the planned vector width and at every narrower one, every access bounds-checked
// — and compared with the definition's loop over (entry, box); every refusal with its reason;
// indices out of range and null arguments. Built with -fsanitize=address,undefined by
// tools/cs_host_sanitize.sh; needs no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ghex_amd/csrc/ghx_addr.hpp"
#include "../../ghex_amd/csrc/ghx_plan.hpp"

#define CHECK(c)                                                                  \
    do                                                                            \
    {                                                                             \
        if (!(c))                                                                 \
        {                                                                         \
            std::printf("%s:%d: CHECK failed: %s (%s)\n", __FILE__, __LINE__, #c, \
                        ghx_last_error());                                        \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

namespace
{
// a field of D spatial dims of extent E (halo H), optional component axis, element strides from
// the layout (layout[d] = D - 1: fastest), fastest stride `fast` elements
struct field
{
    ghx_field_desc d{};
    int64_t n_elems = 0;
};

field make_field(int D, int E, int H, int elem, const int* layout, int ncomp, int fast)
{
    field f;
    const int nd = D + (ncomp ? 1 : 0);
    f.d.dim = nd;
    f.d.elem_size = elem;
    f.d.num_components = ncomp ? ncomp : 1;
    f.d.has_components = ncomp ? 1 : 0;
    int64_t s = fast;
    for (int v = nd - 1; v >= 0; --v)
        for (int d = 0; d < nd; ++d)
            if (layout[d] == v)
            {
                const int ext = d < D ? E : ncomp;
                f.d.layout[d] = v;
                f.d.byte_strides[d] = s * elem;
                f.d.offsets[d] = d < D ? H : 0;
                f.d.extents[d] = ext;
                s *= ext;
            }
    f.n_elems = s;
    return f;
}

ghx_box box3(int x0, int x1, int y0, int y1, int z0, int z1)
{
    ghx_box b{};
    b.first[0] = x0, b.last[0] = x1, b.first[1] = y0, b.last[1] = y1, b.first[2] = z0, b.last[2] = z1;
    return b;
}

// the 26 send boxes and the 26 receive boxes of one periodic N^D domain with halo H
void periodic_boxes(int D, int N, int H, std::vector<ghx_box>& send, std::vector<ghx_box>& recv)
{
    int dir[3];
    const int lo = D > 2 ? -1 : 0, hi = D > 2 ? 1 : 0;
    for (dir[2] = lo; dir[2] <= hi; ++dir[2])
        for (dir[1] = -1; dir[1] <= 1; ++dir[1])
            for (dir[0] = -1; dir[0] <= 1; ++dir[0])
            {
                if (!dir[0] && !dir[1] && !dir[2]) continue;
                ghx_box s{}, r{};
                for (int d = 0; d < D; ++d)
                {
                    r.first[d] = dir[d] < 0 ? -H : dir[d] > 0 ? N : 0;
                    r.last[d] = dir[d] < 0 ? -1 : dir[d] > 0 ? N + H - 1 : N - 1;
                    s.first[d] = dir[d] < 0 ? N - H : 0;
                    s.last[d] = dir[d] > 0 ? H - 1 : N - 1;
                }
                send.push_back(s);
                recv.push_back(r);
            }
}

// element index in the field of a cell of `box`, and the order of the box's cells in its dense
// buffer box: slowest layout dim outermost, component axis included
void box_cells(const ghx_field_desc& f, const ghx_box& b, std::vector<int64_t>& out)
{
    const int D = f.dim, sp = D - (f.has_components ? 1 : 0);
    int order[GHX_MAX_DIM];  // slowest first
    for (int d = 0; d < D; ++d) order[f.layout[d]] = d;
    int64_t first[GHX_MAX_DIM], ext[GHX_MAX_DIM], c[GHX_MAX_DIM] = {};
    int64_t n = 1;
    for (int d = 0; d < D; ++d)
    {
        first[d] = d < sp ? b.first[d] + f.offsets[d] : 0;
        ext[d] = d < sp ? b.last[d] - b.first[d] + 1 : f.num_components;
        n *= ext[d];
    }
    for (int64_t i = 0; i < n; ++i)
    {
        int64_t e = 0;
        for (int d = 0; d < D; ++d) e += (first[d] + c[d]) * (f.byte_strides[d] / f.elem_size);
        out.push_back(e);
        for (int k = D - 1; k >= 0; --k)
        {
            const int d = order[k];
            if (++c[d] < ext[d]) break;
            c[d] = 0;
        }
    }
}

template<typename T>
struct host_state
{
    std::vector<std::vector<T>> fields;
    std::vector<std::vector<T>> bufs;  // in elements from the buffer's first byte
};

// the definition: for (entry, box) ascending, field[cell] += message cell; then zeros
template<typename T>
void definition(host_state<T>& st, const std::vector<ghx_pack_entry>& contrib, const std::vector<ghx_pack_entry>& zero,
                bool zero_halos)
{
    for (const ghx_pack_entry& e : contrib)
    {
        int64_t at = int64_t(e.buffer_offset / sizeof(T));
        for (int b = 0; b < e.n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            box_cells(e.field, e.boxes[b], cells);
            for (int64_t c : cells)
            {
                T& v = st.fields[size_t(e.field_slot)].at(size_t(c));
                v = T(v + st.bufs[size_t(e.buffer_slot)].at(size_t(at++)));
            }
        }
    }
    if (!zero_halos) return;
    for (const ghx_pack_entry& z : zero)
        for (int b = 0; b < z.n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            box_cells(z.field, z.boxes[b], cells);
            for (int64_t c : cells) st.fields[size_t(z.field_slot)].at(size_t(c)) = T(0);
        }
}

// the launch on the host: every tile record at vector width 1 << w (w <= the tile's wlog2, never
// below the element), every vector through sacc_decode, every access checked against its array
template<typename T>
void replay(const ghx::saccum_plan& p, host_state<T>& st, bool zero_halos, int narrow_by)
{
    const size_t n_tiles = zero_halos ? p.tiles.size() : p.n_sum_tiles;
    int elog2 = 0;
    while ((1u << elog2) < sizeof(T)) ++elog2;
    for (size_t t = 0; t < n_tiles; ++t)
    {
        const ghx::sacc_tile& s = p.tiles[t];
        CHECK(s.wlog2 >= elog2 && s.wlog2 <= 4 && s.len % (1u << s.wlog2) == 0 && s.len > 0 && s.n_rows > 0);
        const int w = std::max(elog2, int(s.wlog2) - narrow_by);
        CHECK((t < p.n_sum_tiles) == (s.zero == 0) && (s.zero == 0) == (s.n_src > 0));
        std::vector<T>& F = st.fields.at(s.field_slot);
        const uint32_t nv = ghx::sacc_vectors(s, w);
        CHECK(uint64_t(nv) << w == uint64_t(s.n_rows) * s.len);
        for (uint32_t i = 0; i < nv; ++i)
        {
            uint32_t c[4], col;
            ghx::sacc_decode(s, i, w, c, col);
            CHECK(c[0] < s.ext[0] && c[1] < s.ext[1] && c[2] < s.ext[2] && c[3] < s.ext[3]);
            CHECK(col >= s.col0 && col + (1u << w) <= s.col0 + s.len);
            const int64_t foff = ghx::affine_offset(s.field_off, s.stride, c) + int64_t(col);
            CHECK(foff >= 0 && foff % int64_t(1u << w) == 0);
            for (uint32_t k = 0; k < (1u << w) / sizeof(T); ++k)
            {
                T& cell = F.at(size_t(foff) / sizeof(T) + k);
                if (s.zero)
                {
                    cell = T(0);
                    continue;
                }
                T acc = cell;
                for (uint32_t j = s.first_src; j < s.first_src + s.n_src; ++j)
                {
                    const ghx::sacc_src& r = p.srcs.at(j);
                    CHECK((s.buf_mask >> r.buf_slot) & 1u);
                    const uint64_t boff = r.buf_off + uint64_t(c[0]) * r.stride[0] + uint64_t(c[1]) * r.stride[1] +
                                          uint64_t(c[2]) * r.stride[2] + uint64_t(c[3]) * r.stride[3] + col;
                    CHECK(boff % (1u << w) == 0);
                    acc = T(acc + st.bufs.at(r.buf_slot).at(size_t(boff) / sizeof(T) + k));
                }
                cell = acc;
            }
        }
    }
}

template<typename T>
T value(uint64_t i)
{
    const uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;
    return T(int64_t(h >> 40) % 2001 - 1000);  // integer-valued: every sum is exact and order-free
}

template<typename T>
void fill(host_state<T>& st, const std::vector<field>& fields, const std::vector<size_t>& buf_elems)
{
    for (size_t k = 0; k < fields.size(); ++k)
    {
        st.fields.emplace_back(size_t(fields[k].n_elems));
        for (size_t i = 0; i < st.fields[k].size(); ++i) st.fields[k][i] = value<T>(i * 64 + k);
    }
    for (size_t b = 0; b < buf_elems.size(); ++b)
    {
        st.bufs.emplace_back(buf_elems[b]);
        for (size_t i = 0; i < st.bufs[b].size(); ++i) st.bufs[b][i] = value<T>((i << 8) + 77 * b + 5);
    }
}

template<typename T>
void one_domain(int D, int N, int H, const int* layout, int ncomp, int fast, int32_t code, int64_t n_boxes,
                int64_t max_sources)
{
    const field f = make_field(D, N + 2 * H, H, int(sizeof(T)), layout, ncomp, fast);
    std::vector<ghx_box> send, recv;
    periodic_boxes(D, N, H, send, recv);
    ghx_pack_entry c{}, z{};
    c.field = z.field = f.d;
    c.buffer_offset = 3 * sizeof(T);
    c.boxes = send.data();
    c.n_boxes = int32_t(send.size());
    z.boxes = recv.data();
    z.n_boxes = int32_t(recv.size());
    z.buffer_slot = -5;  // ignored
    size_t msg = 3;
    for (const ghx_box& b : send)
    {
        std::vector<int64_t> cells;
        box_cells(f.d, b, cells);
        msg += cells.size();
    }
    ghx_saccum* p = nullptr;
    CHECK(ghx_saccum_create(&c, &code, 1, &z, 1, &p) == GHX_OK && p);
    uint64_t bytes = 0;
    int64_t nb = 0, nz = 0, ns = 0, mx = 0;
    int32_t nt = 0;
    CHECK(ghx_saccum_info(p, &bytes, &nb, &nz, &ns, &mx, &nt) == GHX_OK);
    CHECK(bytes == (msg - 3) * sizeof(T) && nz == int64_t(recv.size()) && nt >= nb + nz);
    if (n_boxes) CHECK(nb == n_boxes && mx == max_sources);
    for (int64_t k = 0; k < nb + nz; ++k)
    {
        ghx_saccum_box_info bi;
        CHECK(ghx_saccum_box(p, k, &bi) == GHX_OK && bi.field_slot == 0 && bi.zero == (k >= nb ? 1 : 0));
        CHECK(bi.first_src + bi.n_src <= ns && (bi.n_src > 0) == (k < nb));
    }
    for (int64_t j = 0; j < ns; ++j)
    {
        int32_t e = -1, b = -1, s = -1;
        uint64_t off = 0;
        CHECK(ghx_saccum_source(p, j, &e, &b, &s, &off) == GHX_OK && e == 0 && b >= 0 && b < c.n_boxes && s == 0);
        CHECK(off >= c.buffer_offset && off < msg * sizeof(T));
    }
    ghx_saccum_box_info bi;
    CHECK(ghx_saccum_box(p, nb + nz, &bi) == GHX_ERR_INVALID && ghx_saccum_box(p, -1, &bi) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_box(p, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_source(p, ns, nullptr, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_source(p, -1, nullptr, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    for (int zero_halos = 0; zero_halos < 2; ++zero_halos)
        for (int narrow = 0; narrow < 3; ++narrow)
        {
            host_state<T> want, got;
            fill(want, {f}, {msg});
            fill(got, {f}, {msg});
            definition(want, {c}, {z}, zero_halos != 0);
            replay(*p, got, zero_halos != 0, narrow);
            CHECK(want.fields[0] == got.fields[0]);
            host_state<T> before;
            fill(before, {f}, {msg});
            CHECK(before.fields[0] != got.fields[0] && before.bufs[0] == got.bufs[0]);
        }
    // without a device the plan cannot run; wrong pointer arrays are refused before that
    CHECK(ghx_saccum_execute(p, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_destroy(p) == GHX_OK);
}

void sixty_four_slots()
{
    // slot s: a 2-D field of its own size and element type, its messages in buffer 63 - s
    const int lay_x[2] = {1, 0}, lay_y[2] = {0, 1};
    std::vector<field> fields;
    std::vector<std::vector<ghx_box>> send(64), recv(64);
    std::vector<ghx_pack_entry> contrib, zero;
    std::vector<int32_t> dt;
    for (int s = 0; s < 64; ++s)
    {
        const int N = 3 + s % 4, H = 1 + s % 2;
        fields.push_back(make_field(2, N + 2 * H, H, 8, s % 3 ? lay_x : lay_y, 0, 1));
        periodic_boxes(2, N, H, send[size_t(s)], recv[size_t(s)]);
    }
    std::vector<size_t> buf_elems(64);
    for (int s = 0; s < 64; ++s)
    {
        ghx_pack_entry c{}, z{};
        c.field = z.field = fields[size_t(s)].d;
        c.field_slot = z.field_slot = s;
        c.buffer_slot = 63 - s;
        c.buffer_offset = uint64_t(s % 5) * 8;
        c.boxes = send[size_t(s)].data();
        c.n_boxes = int32_t(send[size_t(s)].size());
        z.boxes = recv[size_t(s)].data();
        z.n_boxes = int32_t(recv[size_t(s)].size());
        size_t n = size_t(s % 5);
        for (const ghx_box& b : send[size_t(s)])
        {
            std::vector<int64_t> cells;
            box_cells(c.field, b, cells);
            n += cells.size();
        }
        buf_elems[size_t(63 - s)] = n;
        contrib.push_back(c);
        zero.push_back(z);
        dt.push_back(s % 2 ? GHX_DT_I64 : GHX_DT_F64);
    }
    ghx_saccum* p = nullptr;
    CHECK(ghx_saccum_create(contrib.data(), dt.data(), 64, zero.data(), 64, &p) == GHX_OK && p);
    int64_t nb = 0, nz = 0;
    CHECK(ghx_saccum_info(p, nullptr, &nb, &nz, nullptr, nullptr, nullptr) == GHX_OK && nb >= 64 && nz == 64 * 8);
    // every value is an integer below 2^53: the double replay equals the uint64 one
    host_state<double> want, got;
    fill(want, fields, buf_elems);
    fill(got, fields, buf_elems);
    definition(want, contrib, zero, true);
    replay(*p, got, true, 0);
    for (size_t s = 0; s < 64; ++s) CHECK(want.fields[s] == got.fields[s]);
    CHECK(ghx_saccum_destroy(p) == GHX_OK);
}

void refused(const std::vector<ghx_pack_entry>& c, const std::vector<int32_t>& dt, const std::vector<ghx_pack_entry>& z,
             const char* fragment)
{
    ghx_saccum* p = reinterpret_cast<ghx_saccum*>(1);
    CHECK(ghx_saccum_create(c.data(), dt.data(), int32_t(c.size()), z.data(), int32_t(z.size()), &p) ==
          GHX_ERR_INVALID);
    CHECK(p == nullptr);
    if (!std::strstr(ghx_last_error(), fragment))
    {
        std::printf("refusal '%s' lacks '%s'\n", ghx_last_error(), fragment);
        std::exit(1);
    }
}

void refusals()
{
    const int lay[3] = {2, 1, 0}, yx[3] = {1, 2, 0};
    const field f = make_field(3, 6, 1, 8, lay, 0, 1), f4 = make_field(3, 6, 1, 4, lay, 0, 1);
    const ghx_box own = box3(0, 0, 0, 3, 0, 3), halo = box3(-1, -1, 0, 3, 0, 3);
    auto entry = [](const field& fl, const ghx_box* b, int fslot, int bslot, uint64_t off) {
        ghx_pack_entry e{};
        e.field = fl.d;
        e.field_slot = fslot;
        e.buffer_slot = bslot;
        e.buffer_offset = off;
        e.boxes = b;
        e.n_boxes = 1;
        return e;
    };
    const ghx_pack_entry ok = entry(f, &own, 0, 0, 0);
    refused({ok}, {0}, {}, "unknown dtype code");
    refused({ok}, {5}, {}, "unknown dtype code");
    refused({ok}, {GHX_DT_F32}, {}, "elem_size is 8");
    refused({entry(f4, &own, 0, 0, 0)}, {GHX_DT_F64}, {}, "elem_size is 4");
    refused({ok}, {GHX_DT_F64}, {entry(make_field(3, 6, 1, 2, lay, 0, 1), &halo, 1, 0, 0)}, "zero entry's elem_size is 2");
    refused({entry(f, &own, 64, 0, 0)}, {GHX_DT_F64}, {}, "at most 64 field and 64 buffer slots");
    refused({entry(f, &own, 0, 64, 0)}, {GHX_DT_F64}, {}, "at most 64 field and 64 buffer slots");
    refused({ok}, {GHX_DT_F64}, {entry(f, &halo, 64, 0, 0)}, "at most 64 field and 64 buffer slots");
    refused({entry(f, &own, -1, 0, 0)}, {GHX_DT_F64}, {}, "negative slot");
    refused({entry(f, &own, 0, -1, 0)}, {GHX_DT_F64}, {}, "negative slot");
    refused({ok, entry(make_field(3, 6, 1, 8, yx, 0, 1), &own, 0, 1, 0)}, {GHX_DT_F64, GHX_DT_F64}, {},
            "differ in their field descriptor");
    refused({ok}, {GHX_DT_F64}, {entry(make_field(3, 7, 1, 8, lay, 0, 1), &halo, 0, 0, 0)}, "differ in their field descriptor");
    refused({ok, entry(f, &own, 0, 1, 0)}, {GHX_DT_F64, GHX_DT_I64}, {}, "differ in their dtype");
    refused({entry(f, &own, 0, 0, 12)}, {GHX_DT_F64}, {}, "not a multiple of the element size");
    const ghx_box meets = box3(0, 1, 3, 4, 3, 4);
    refused({ok}, {GHX_DT_F64}, {entry(f, &meets, 0, 0, 0)}, "is both summed and zeroed");
    const ghx_box outside = box3(0, 5, 0, 3, 0, 3), below = box3(-2, 0, 0, 3, 0, 3), empty = box3(2, 1, 0, 3, 0, 3);
    refused({entry(f, &outside, 0, 0, 0)}, {GHX_DT_F64}, {}, "outside the field extents");
    refused({ok}, {GHX_DT_F64}, {entry(f, &below, 1, 0, 0)}, "outside the field extents");
    refused({entry(f, &empty, 0, 0, 0)}, {GHX_DT_F64}, {}, "first must be <= last");
    ghx_pack_entry bad = ok;
    bad.field.byte_strides[1] += 4;
    refused({bad}, {GHX_DT_F64}, {}, "byte stride of the field is not a multiple");
    bad = ok;
    bad.boxes = nullptr;
    refused({bad}, {GHX_DT_F64}, {}, "bad boxes");
    bad = ok;
    bad.n_boxes = -1;
    refused({bad}, {GHX_DT_F64}, {}, "bad boxes");
    bad = ok;
    bad.field.layout[0] = 1;
    refused({bad}, {GHX_DT_F64}, {}, "permutation");
    // overlapping buffer ranges are fine: contributions are only read
    const ghx_pack_entry two[2] = {ok, entry(f, &own, 1, 0, 8)};
    const int32_t dt[2] = {GHX_DT_F64, GHX_DT_F64};
    ghx_saccum* p = nullptr;
    CHECK(ghx_saccum_create(two, dt, 2, nullptr, 0, &p) == GHX_OK && p);
    CHECK(ghx_saccum_destroy(p) == GHX_OK);
    // null arguments
    CHECK(ghx_saccum_create(nullptr, nullptr, 1, nullptr, 0, &p) == GHX_ERR_INVALID && p == nullptr);
    CHECK(ghx_saccum_create(two, nullptr, 2, nullptr, 0, &p) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_create(two, dt, 2, nullptr, 1, &p) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_create(two, dt, -1, nullptr, 0, &p) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_create(two, dt, 2, nullptr, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_execute(nullptr, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_destroy(nullptr) == GHX_OK);
    // an empty plan has nothing to launch
    CHECK(ghx_saccum_create(nullptr, nullptr, 0, nullptr, 0, &p) == GHX_OK && p);
    CHECK(ghx_saccum_execute(p, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_OK);
    CHECK(ghx_saccum_destroy(p) == GHX_OK);
}
}  // namespace

int main()
{
    const int xyz[3] = {2, 1, 0}, zyx[3] = {0, 1, 2}, yzx[3] = {1, 2, 0};
    const int comp_fast[4] = {2, 1, 0, 3}, comp_slow[4] = {3, 2, 1, 0}, xy[2] = {1, 0};
    one_domain<uint64_t>(3, 3, 2, xyz, 0, 1, GHX_DT_I64, 27, 26);
    one_domain<uint32_t>(3, 3, 2, zyx, 0, 1, GHX_DT_I32, 27, 26);
    one_domain<double>(3, 3, 2, yzx, 0, 1, GHX_DT_F64, 27, 26);
    one_domain<float>(3, 3, 2, comp_fast, 3, 1, GHX_DT_F32, 27, 26);
    one_domain<uint32_t>(3, 3, 2, comp_slow, 2, 1, GHX_DT_I32, 27, 26);
    one_domain<double>(3, 3, 2, xyz, 0, 2, GHX_DT_F64, 27, 26);   // strided fastest dim
    one_domain<double>(3, 6, 2, xyz, 0, 1, GHX_DT_F64, 26, 7);
    one_domain<float>(3, 5, 3, xyz, 0, 1, GHX_DT_F32, 0, 26);
    one_domain<uint64_t>(3, 2, 2, xyz, 0, 1, GHX_DT_I64, 1, 26);
    one_domain<float>(2, 7, 2, xy, 0, 1, GHX_DT_F32, 8, 3);
    ghx_tune("tile_bytes", 1024);  // several tiles per sub-box, a tile ending inside one
    one_domain<double>(3, 19, 2, xyz, 0, 1, GHX_DT_F64, 26, 7);
    one_domain<float>(2, 300, 2, xy, 0, 1, GHX_DT_F32, 8, 3);     // rows longer than a tile
    ghx_tune("reset", 0);
    sixty_four_slots();
    refusals();
    std::printf("saccum_host_check: OK\n");
    return 0;
}
