// uplan_segment_host_check — stand-alone host program (its own main; links the library's sources)
// for ghx_uplan_segment: index-list plans of every row form (seg_u::mode 0, 1, 2), int32 and
// int64 lid tables, a list split below 2^30 bytes and 130 slots in three launch groups are
// created without a device, and every segment is read back and compared with the entry it came
// from; indices out of range and null arguments are refused. Built with
// -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ghx.h"

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
ghx_upack_entry entry(int elem, int levels, int first, int64_t is, int64_t ls, int fslot, int bslot,
                      uint64_t boff, const std::vector<int64_t>& lids)
{
    ghx_upack_entry e{};
    e.data.elem_size = elem;
    e.data.levels = levels;
    e.data.levels_first = first;
    e.data.index_stride = is;
    e.data.level_stride = ls;
    e.field_slot = fslot;
    e.buffer_slot = bslot;
    e.buffer_offset = boff;
    e.lids = lids.data();
    e.n_lids = int64_t(lids.size());
    return e;
}

std::vector<int64_t> some_lids(int64_t n, int64_t bias)
{
    std::vector<int64_t> l(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) l[size_t(i)] = (i * 7919) % 10007 + bias;
    return l;
}

int n_segments(const ghx_uplan* p)
{
    int32_t n = -1;
    CHECK(ghx_uplan_info(p, nullptr, &n, nullptr) == GHX_OK);
    return n;
}

void every_form()
{
    const auto a = some_lids(3001, 0), b = some_lids(3002, 0), c = some_lids(3003, (int64_t(1) << 31) + 5);
    const ghx_upack_entry ents[4] = {
        entry(8, 3, 1, 4, 1, 0, 0, 0, a),        // mode 0: 24-B rows
        entry(4, 3, 1, 5, 2, 1, 1, 8, b),        // mode 1
        entry(16, 3, 0, 1, 10010, 2, 2, 16, c),  // mode 2, int64 table
        entry(4, 1, 1, 1, 1, 3, 3, 32, a),       // mode 0, run-eligible
    };
    for (int dir = 0; dir < 2; ++dir)
    {
        ghx_uplan* p = nullptr;
        CHECK(ghx_uplan_create(ents, 4, dir, &p) == GHX_OK);
        CHECK(n_segments(p) == 4);
        const int mode[4] = {0, 1, 2, 0}, wlog2[4] = {3, 2, 4, 2}, lid64[4] = {0, 0, 1, 0};
        const uint32_t row[4] = {24, 4, 16, 4};
        for (int k = 0; k < 4; ++k)
        {
            ghx_usegment_info s;
            CHECK(ghx_uplan_segment(p, k, &s) == GHX_OK);
            const auto& d = ents[k].data;
            CHECK(s.mode == mode[k] && s.wlog2 == wlog2[k] && s.lid64 == lid64[k]);
            CHECK(s.row_bytes == row[k] && s.n == uint32_t(ents[k].n_lids));
            CHECK(s.bytes == uint32_t(ents[k].n_lids * d.levels * d.elem_size));
            CHECK(s.tile_bytes > 0 && s.tile_bytes % s.row_bytes == 0);
            CHECK(s.field_slot == k && s.buffer_slot == k && s.buf_off == ents[k].buffer_offset);
            CHECK(s.index_stride_b == d.index_stride * d.elem_size);
            CHECK(s.level_stride_b == d.level_stride * d.elem_size && s.field_off == 0);
            CHECK((s.runs != 0) == (k == 3) && s.fpol == 0);
        }
        ghx_usegment_info s;
        CHECK(ghx_uplan_segment(p, 4, &s) == GHX_ERR_INVALID);
        CHECK(ghx_uplan_segment(p, -1, &s) == GHX_ERR_INVALID);
        CHECK(ghx_uplan_segment(p, 0, nullptr) == GHX_ERR_INVALID);
        CHECK(ghx_uplan_segment(nullptr, 0, &s) == GHX_ERR_INVALID);
        CHECK(ghx_uplan_destroy(p) == GHX_OK);
    }
}

// a levels-last list of more than 2^30 bytes is planned level by level as mode-0 segments
void split_list()
{
    const int64_t n = (int64_t(1) << 26) + 3;  // x 16 B x 2 levels > 2^30
    std::vector<int64_t> l(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) l[size_t(i)] = i;
    const ghx_upack_entry e = entry(16, 2, 0, 1, n + 1, 0, 0, 0, l);
    ghx_uplan* p = nullptr;
    CHECK(ghx_uplan_create(&e, 1, 0, &p) == GHX_OK);
    const int ns = n_segments(p);
    CHECK(ns == 4);
    uint64_t covered = 0;
    for (int k = 0; k < ns; ++k)
    {
        ghx_usegment_info s;
        CHECK(ghx_uplan_segment(p, k, &s) == GHX_OK);
        CHECK(s.mode == 0 && s.row_bytes == 16 && s.buf_off == covered);
        CHECK(s.field_off == (k / 2) * (n + 1) * 16);
        covered += s.bytes;
    }
    CHECK(covered == uint64_t(n) * 32);
    CHECK(ghx_uplan_destroy(p) == GHX_OK);
}

void many_slots()
{
    constexpr int N = 130;
    const auto l = some_lids(4, 0);
    std::vector<ghx_upack_entry> ents;
    for (int k = 0; k < N; ++k) ents.push_back(entry(4, 2, 1, 2, 1, k, N - 1 - k, 0, l));
    ghx_uplan* p = nullptr;
    CHECK(ghx_uplan_create(ents.data(), N, 1, &p) == GHX_OK);
    CHECK(n_segments(p) == N);
    for (int k = 0; k < N; ++k)
    {
        ghx_usegment_info s;
        CHECK(ghx_uplan_segment(p, k, &s) == GHX_OK);
        CHECK(s.field_slot == k && s.buffer_slot == N - 1 - k && s.bytes == 32 && s.mode == 0);
    }
    ghx_usegment_info s;
    CHECK(ghx_uplan_segment(p, N, &s) == GHX_ERR_INVALID);
    CHECK(ghx_uplan_destroy(p) == GHX_OK);
}
}  // namespace

int main()
{
    every_form();
    split_list();
    many_slots();
    std::printf("uplan_segment_host_check: ok\n");
    return 0;
}
