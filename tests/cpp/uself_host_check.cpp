// uself_host_check — stand-alone host program (its own main; links the library's sources) for the
// fused index-list self exchange plan: ghx_uself_create / _info / _segment / _destroy through the
// C header, created without a device. Plans of every row form, int32 and int64 tables per side,
// a buffer offset that narrows the vector width, a list split below 2^30 bytes; every refusal
// with its reason; indices out of range and null arguments. Built with
// -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// n distinct lids: (i * 7919) % 10007 is a permutation of the residues for i < 10007
std::vector<int64_t> some_lids(int64_t n, int64_t first, int64_t bias)
{
    std::vector<int64_t> l(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) l[size_t(i)] = ((first + i) * 7919) % 10007 + bias;
    return l;
}

void every_form()
{
    const int64_t big = (int64_t(1) << 31) + 5;
    const auto s0 = some_lids(3001, 0, 0), t0 = some_lids(3001, 5000, 0);
    const auto s1 = some_lids(3002, 0, 0), t1 = some_lids(3002, 5000, big);
    const auto s2 = some_lids(3003, 0, big), t2 = some_lids(3003, 5000, 0);
    const ghx_upack_entry src[4] = {
        entry(8, 3, 1, 4, 1, 0, 0, 0, s0),        // mode 0: 24-B rows, padded source
        entry(4, 3, 1, 3, 1, 1, 1, 8, s1),        // contiguous against strided levels: mode 1
        entry(16, 3, 0, 1, 10010, 2, 2, 20, s2),  // mode 2, offset 20 narrows 16-B elements to 4 B
        entry(4, 1, 1, 1, 1, 3, 2, 3003 * 48 + 32, s0),  // run-eligible, second message of buffer 2
    };
    const ghx_upack_entry dst[4] = {
        entry(8, 3, 1, 3, 1, 4, 0, 0, t0),
        entry(4, 3, 1, 1, 10007, 5, 1, 8, t1),
        entry(16, 3, 0, 1, 10007, 6, 2, 20, t2),
        entry(4, 1, 1, 1, 1, 7, 2, 3003 * 48 + 32, t0),
    };
    ghx_uself* p = nullptr;
    CHECK(ghx_uself_create(src, dst, 4, &p) == GHX_OK && p);
    uint64_t bytes = 0;
    int32_t ns = -1, nt = -1;
    CHECK(ghx_uself_info(p, &bytes, &ns, &nt) == GHX_OK);
    CHECK(ns == 4 && bytes == 3001u * 24 + 3002u * 12 + 3003u * 48 + 3001u * 4);
    const int mode[4] = {0, 1, 2, 0}, wlog2[4] = {3, 2, 2, 2};
    const int s64[4] = {0, 0, 1, 0}, d64[4] = {0, 1, 0, 0};
    const uint32_t row[4] = {24, 4, 16, 4};
    int32_t tiles = 0;
    for (int k = 0; k < 4; ++k)
    {
        ghx_uself_segment_info s;
        CHECK(ghx_uself_segment(p, k, &s) == GHX_OK);
        CHECK(s.message == k && s.n_segments == 4 && s.first_index == 0);
        CHECK(s.mode == mode[k] && s.wlog2 == wlog2[k] && s.row_bytes == row[k]);
        CHECK(s.src_lid64 == s64[k] && s.dst_lid64 == d64[k]);
        CHECK(s.n == uint32_t(src[k].n_lids));
        CHECK(s.bytes == uint32_t(src[k].n_lids * src[k].data.levels * src[k].data.elem_size));
        CHECK(s.tile_bytes > 0 && s.tile_bytes % s.row_bytes == 0);
        CHECK(s.src_slot == src[k].field_slot && s.dst_slot == dst[k].field_slot);
        CHECK(s.buf_slot == src[k].buffer_slot && s.buf_off == src[k].buffer_offset);
        CHECK(s.src_index_stride_b == src[k].data.index_stride * src[k].data.elem_size);
        CHECK(s.dst_level_stride_b == dst[k].data.level_stride * dst[k].data.elem_size);
        CHECK((s.src_runs != 0) == (k == 3) && (s.dst_runs != 0) == (k == 3));
        tiles += int32_t((s.bytes + s.tile_bytes - 1) / s.tile_bytes);
    }
    CHECK(tiles == nt);
    ghx_uself_segment_info s;
    CHECK(ghx_uself_segment(p, 4, &s) == GHX_ERR_INVALID);
    CHECK(ghx_uself_segment(p, -1, &s) == GHX_ERR_INVALID);
    CHECK(ghx_uself_segment(p, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uself_segment(nullptr, 0, &s) == GHX_ERR_INVALID);
    CHECK(ghx_uself_info(nullptr, &bytes, &ns, &nt) == GHX_ERR_INVALID);
    // too few pointers: refused before anything is launched
    void* one[1] = {reinterpret_cast<void*>(4096)};
    CHECK(ghx_uself_execute(p, one, 1, one, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
    CHECK(ghx_uself_destroy(nullptr) == GHX_OK);
    // an empty plan
    CHECK(ghx_uself_create(nullptr, nullptr, 0, &p) == GHX_OK && p);
    CHECK(ghx_uself_info(p, &bytes, &ns, &nt) == GHX_OK && bytes == 0 && ns == 0 && nt == 0);
    CHECK(ghx_uself_execute(p, one, 1, one, 1, nullptr) == GHX_OK);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
}

// a levels-last list of more than 2^30 bytes: level by level on both sides and in the buffer
void split_list()
{
    const int64_t n = (int64_t(1) << 20) + 3;  // x 1 KiB x 2 levels > 2^30: two pieces per level
    std::vector<int64_t> s(static_cast<size_t>(n)), t(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i)
    {
        s[size_t(i)] = i;
        t[size_t(i)] = n - 1 - i;
    }
    const uint64_t off = 256;
    const ghx_upack_entry se = entry(1024, 2, 0, 1, n + 1, 0, 0, off, s);
    const ghx_upack_entry de = entry(1024, 2, 0, 1, n + 5, 1, 0, off, t);
    ghx_uself* p = nullptr;
    CHECK(ghx_uself_create(&se, &de, 1, &p) == GHX_OK);
    int32_t ns = -1;
    CHECK(ghx_uself_info(p, nullptr, &ns, nullptr) == GHX_OK && ns == 4);
    uint64_t covered = 0;
    for (int k = 0; k < ns; ++k)
    {
        ghx_uself_segment_info g;
        CHECK(ghx_uself_segment(p, k, &g) == GHX_OK);
        CHECK(g.mode == 0 && g.row_bytes == 1024 && g.buf_off == off + covered && g.buf_slot == 0);
        CHECK(g.src_field_off == (k / 2) * (n + 1) * 1024 && g.dst_field_off == (k / 2) * (n + 5) * 1024);
        CHECK(g.buf_off == off + uint64_t((k / 2) * n + g.first_index) * 1024);
        covered += g.bytes;
    }
    CHECK(covered == uint64_t(n) * 2048);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
}

void refused(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n, const char* why)
{
    ghx_uself* p = reinterpret_cast<ghx_uself*>(8);
    CHECK(ghx_uself_create(src, dst, n, &p) == GHX_ERR_INVALID);
    CHECK(p == nullptr);
    if (!std::strstr(ghx_last_error(), why))
    {
        std::printf("refusal reason '%s' lacks '%s'\n", ghx_last_error(), why);
        std::exit(1);
    }
}

void refusals()
{
    const auto s = some_lids(300, 0, 0), t = some_lids(300, 5000, 0), u = some_lids(299, 5000, 0);
    const auto s2 = some_lids(40, 400, 0), t2 = some_lids(40, 6000, 0);
    auto one = [&](const ghx_upack_entry& a, const ghx_upack_entry& b, const char* why) {
        refused(&a, &b, 1, why);
    };
    const char* same = "do not describe the same message bytes";
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 0, u), same);
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(4, 1, 1, 1, 1, 1, 0, 0, t), same);
    one(entry(4, 2, 1, 2, 1, 0, 0, 0, s), entry(4, 3, 1, 3, 1, 1, 0, 0, t), same);
    one(entry(4, 2, 1, 2, 1, 0, 0, 0, s), entry(4, 2, 0, 1, 10007, 1, 0, 0, t), same);
    const char* place = "differ in buffer slot or buffer offset";
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 1, 0, t), place);
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 16, t), place);
    {
        const ghx_upack_entry a[2] = {entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 0, 0, 2392, s2)};
        const ghx_upack_entry b[2] = {entry(8, 1, 1, 1, 1, 1, 0, 0, t), entry(8, 1, 1, 1, 1, 1, 0, 2392, t2)};
        refused(a, b, 2, "two messages overlap in one buffer");
    }
    auto neg = s;
    neg[17] = -1;
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, neg), entry(8, 1, 1, 1, 1, 1, 0, 0, t), "negative local index");
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 0, neg), "negative local index");
    one(entry(0, 1, 1, 1, 1, 0, 0, 0, s), entry(0, 1, 1, 1, 1, 1, 0, 0, t), "bad unstructured data descriptor");
    one(entry(8, 0, 1, 1, 1, 0, 0, 0, s), entry(8, 0, 1, 1, 1, 1, 0, 0, t), "bad unstructured data descriptor");
    one(entry(8, 1, 1, 1, 1, -1, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 0, t), "negative slot");
    one(entry(8, 1, 1, 1, 1, 0, -1, 0, s), entry(8, 1, 1, 1, 1, 1, -1, 0, t), "negative slot");
    const char* limit = "at most 64 field and 64 buffer slots";
    one(entry(8, 1, 1, 1, 1, 64, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 0, t), limit);
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 64, 0, 0, t), limit);
    one(entry(8, 1, 1, 1, 1, 0, 64, 0, s), entry(8, 1, 1, 1, 1, 1, 64, 0, t), limit);
    one(entry(1 << 20, 1025, 1, 1025, 1, 0, 0, 0, s), entry(1 << 20, 1025, 1, 1025, 1, 1, 0, 0, t),
        "row of more than 1 GiB");
    // a cell read and written; a cell written twice
    auto hit = t;
    hit[9] = s[250];
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 0, 0, 0, hit), "both a source and a target");
    auto dup = t;
    dup[9] = dup[250];
    one(entry(8, 1, 1, 1, 1, 0, 0, 0, s), entry(8, 1, 1, 1, 1, 1, 0, 0, dup), "appears twice");
    // what patterns do is accepted: the same slot on disjoint cells, repeated source lids
    auto rep = s;
    rep[3] = rep[200];
    ghx_uself* p = nullptr;
    const ghx_upack_entry a = entry(8, 1, 1, 1, 1, 0, 0, 0, rep), b = entry(8, 1, 1, 1, 1, 0, 0, 0, t);
    CHECK(ghx_uself_create(&a, &b, 1, &p) == GHX_OK);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
    CHECK(ghx_uself_create(&a, &b, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uself_create(nullptr, nullptr, 1, &p) == GHX_ERR_INVALID);
    CHECK(ghx_uself_create(&a, &b, -1, &p) == GHX_ERR_INVALID);
}
}  // namespace

int main()
{
    every_form();
    split_list();
    refusals();
    std::printf("uself_host_check: ok\n");
    return 0;
}
