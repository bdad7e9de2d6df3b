// uaccum_host_check — stand-alone host program (its own main; links the library's sources) for the
// adjoint accumulate plan: ghx_uaccum_create / _info / _dest / _contrib / _destroy through the C
// header, created without a device. The tables of a plan with repeated cells, a cell in two
// messages, int64 lids and both buffer layouts; a plan over all 64 field and buffer slots; every
// refusal with its reason; indices out of range and null arguments. Built with
// -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
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

struct plan_tables
{
    uint64_t bytes = 0;
    int64_t n_dest = 0, n_zero = 0, n_contrib = 0, max_per = 0;
    int32_t n_tiles = 0;
    std::vector<ghx_uaccum_dest_info> dest;
    std::vector<std::pair<int32_t, int64_t>> rec;
};

plan_tables read_back(const ghx_uaccum* p)
{
    plan_tables t;
    CHECK(ghx_uaccum_info(p, &t.bytes, &t.n_dest, &t.n_zero, &t.n_contrib, &t.max_per, &t.n_tiles) == GHX_OK);
    for (int64_t k = 0; k < t.n_dest + t.n_zero; ++k)
    {
        ghx_uaccum_dest_info d;
        CHECK(ghx_uaccum_dest(p, k, &d) == GHX_OK);
        t.dest.push_back(d);
    }
    for (int64_t j = 0; j < t.n_contrib; ++j)
    {
        int32_t e = -1;
        int64_t pos = -1;
        CHECK(ghx_uaccum_contrib(p, j, &e, &pos) == GHX_OK);
        t.rec.emplace_back(e, pos);
    }
    ghx_uaccum_dest_info d;
    CHECK(ghx_uaccum_dest(p, t.n_dest + t.n_zero, &d) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_dest(p, -1, &d) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_dest(p, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_contrib(p, t.n_contrib, nullptr, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_contrib(p, -1, nullptr, nullptr) == GHX_ERR_INVALID);
    return t;
}

void tables()
{
    const int64_t big = (int64_t(1) << 31) + 5;
    auto s0 = some_lids(3001, 0, 0);
    for (size_t i = 1; i < 2000; i += 7) s0[i] = s0[0];  // one cell 286 more times
    const auto s1 = some_lids(3002, 100, 0);
    auto s2 = some_lids(3003, 4000, 0);
    s2.back() = s1.back();                               // a cell in two messages
    const auto s3 = some_lids(500, 0, big);              // int64 table
    const auto t0 = some_lids(3001, 5000, 0), t1 = some_lids(3002, 2000, 0);
    const ghx_upack_entry contrib[4] = {
        entry(8, 3, 1, 4, 1, 0, 0, 0, s0),               // levels first, padded rows
        entry(4, 2, 0, 1, 10007, 1, 0, 3001 * 24, s1),   // levels last
        entry(4, 2, 0, 1, 10007, 1, 1, 4, s2),           // same field, element-aligned offset
        entry(8, 1, 1, 1, 1, 2, 1, 3003 * 8 + 8, s3),
    };
    const int32_t dt[4] = {GHX_DT_F64, GHX_DT_I32, GHX_DT_I32, GHX_DT_I64};
    const ghx_upack_entry zero[3] = {
        entry(8, 3, 1, 3, 1, 3, 0, 0, t0),
        entry(4, 2, 0, 1, 10007, 4, 0, 0, t1),
        entry(4, 2, 0, 1, 10007, 4, -7, 0, t0),          // buffer members ignored; overlaps t1's cells
    };
    ghx_uaccum* p = nullptr;
    CHECK(ghx_uaccum_create(contrib, dt, 4, zero, 3, &p) == GHX_OK && p);
    const plan_tables t = read_back(p);
    CHECK(t.n_contrib == 3001 + 3002 + 3003 + 500);
    CHECK(t.bytes == 3001u * 24 + 3002u * 8 + 3003u * 8 + 500u * 8);
    // the expectation: cells -> records in (entry, position) order
    std::map<std::pair<int32_t, int64_t>, std::vector<std::pair<int32_t, int64_t>>> cells;
    for (int32_t e = 0; e < 4; ++e)
        for (int64_t i = 0; i < contrib[e].n_lids; ++i)
            cells[{contrib[e].field_slot, contrib[e].lids[i]}].emplace_back(e, i);
    CHECK(t.n_dest == int64_t(cells.size()));
    int64_t at = 0, most = 0;
    auto it = cells.begin();
    for (int64_t k = 0; k < t.n_dest; ++k, ++it)
    {
        const ghx_uaccum_dest_info& d = t.dest[size_t(k)];
        CHECK(d.zero == 0 && d.field_slot == it->first.first && d.lid == it->first.second);
        CHECK(d.first == at && d.count == int64_t(it->second.size()));
        for (int64_t j = 0; j < d.count; ++j) CHECK(t.rec[size_t(at + j)] == it->second[size_t(j)]);
        at += d.count;
        most = std::max(most, d.count);
    }
    CHECK(at == t.n_contrib && most == t.max_per && most == 287);
    CHECK((cells[{1, s1.back()}].size() == 2));
    std::vector<std::pair<int32_t, int64_t>> z;
    for (const ghx_upack_entry& e : zero)
        for (int64_t i = 0; i < e.n_lids; ++i) z.emplace_back(e.field_slot, e.lids[i]);
    std::sort(z.begin(), z.end());
    z.erase(std::unique(z.begin(), z.end()), z.end());
    CHECK(t.n_zero == int64_t(z.size()));
    for (int64_t k = 0; k < t.n_zero; ++k)
    {
        const ghx_uaccum_dest_info& d = t.dest[size_t(t.n_dest + k)];
        CHECK(d.zero == 1 && d.count == 0 && d.field_slot == z[size_t(k)].first && d.lid == z[size_t(k)].second);
    }
    CHECK(t.n_tiles > 0);
    // without a device the plan cannot run; wrong pointer arrays are refused before that
    CHECK(ghx_uaccum_execute(p, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_destroy(p) == GHX_OK);
}

void sixty_four_slots()
{
    std::vector<std::vector<int64_t>> lids;
    lids.reserve(128);
    for (int s = 0; s < 64; ++s) lids.push_back(some_lids(40 + s, s * 50, 0));
    std::vector<ghx_upack_entry> contrib, zero;
    std::vector<int32_t> dt;
    for (int s = 0; s < 64; ++s)
    {
        const bool wide = s % 2 == 0;
        contrib.push_back(entry(wide ? 8 : 4, 2, s % 3 == 0, s % 3 == 0 ? 2 : 1, s % 3 == 0 ? 1 : 10007, s, 63 - s,
                                uint64_t(s) * 8, lids[size_t(s)]));
        dt.push_back(wide ? (s % 4 == 0 ? GHX_DT_F64 : GHX_DT_I64) : (s % 4 == 1 ? GHX_DT_F32 : GHX_DT_I32));
        // the zero cells of slot s: its own list shifted off its cells
        lids.push_back(std::vector<int64_t>(lids[size_t(s)]));
        for (int64_t& l : lids.back()) l += 20000;
    }
    for (int s = 0; s < 64; ++s)
    {
        ghx_upack_entry z = contrib[size_t(s)];
        z.lids = lids[size_t(64 + s)].data();
        zero.push_back(z);
    }
    ghx_uaccum* p = nullptr;
    CHECK(ghx_uaccum_create(contrib.data(), dt.data(), 64, zero.data(), 64, &p) == GHX_OK && p);
    const plan_tables t = read_back(p);
    int64_t n = 0;
    for (int s = 0; s < 64; ++s) n += 40 + s;
    CHECK(t.n_dest == n && t.n_zero == n && t.n_contrib == n && t.max_per == 1);
    CHECK(t.n_tiles == 128);  // one sum tile and one zero tile per field slot
    CHECK(t.dest.front().field_slot == 0 && t.dest[size_t(n - 1)].field_slot == 63);
    CHECK(ghx_uaccum_destroy(p) == GHX_OK);
}

void refused(const std::vector<ghx_upack_entry>& c, const std::vector<int32_t>& dt, const std::vector<ghx_upack_entry>& z,
             const char* fragment)
{
    ghx_uaccum* p = reinterpret_cast<ghx_uaccum*>(1);
    CHECK(ghx_uaccum_create(c.data(), dt.data(), int32_t(c.size()), z.data(), int32_t(z.size()), &p) ==
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
    const auto l = some_lids(10, 0, 0), m = some_lids(10, 20, 0);
    const std::vector<int64_t> neg = {3, -1};
    const auto ok = entry(8, 3, 1, 3, 1, 0, 0, 0, l);
    refused({ok}, {0}, {}, "unknown dtype code");
    refused({ok}, {5}, {}, "unknown dtype code");
    refused({ok}, {GHX_DT_F32}, {}, "elem_size is 8");
    refused({entry(4, 1, 1, 1, 1, 0, 0, 0, l)}, {GHX_DT_F64}, {}, "elem_size is 4");
    refused({ok}, {GHX_DT_F64}, {entry(2, 1, 1, 1, 1, 1, 0, 0, l)}, "zero entry's elem_size is 2");
    refused({entry(8, 3, 1, 3, 1, 64, 0, 0, l)}, {GHX_DT_F64}, {}, "at most 64 field and 64 buffer slots");
    refused({entry(8, 3, 1, 3, 1, 0, 64, 0, l)}, {GHX_DT_F64}, {}, "at most 64 field and 64 buffer slots");
    refused({ok}, {GHX_DT_F64}, {entry(8, 3, 1, 3, 1, 64, 0, 0, l)}, "at most 64 field and 64 buffer slots");
    refused({entry(8, 3, 1, 3, 1, -1, 0, 0, l)}, {GHX_DT_F64}, {}, "negative slot");
    refused({entry(8, 3, 1, 3, 1, 0, -1, 0, l)}, {GHX_DT_F64}, {}, "negative slot");
    refused({entry(8, 0, 1, 3, 1, 0, 0, 0, l)}, {GHX_DT_F64}, {}, "levels < 1");
    refused({entry(8, 3, 1, 3, 1, 0, 0, 0, neg)}, {GHX_DT_F64}, {}, "negative local index");
    refused({ok}, {GHX_DT_F64}, {entry(8, 3, 1, 3, 1, 1, 0, 0, neg)}, "negative local index");
    refused({entry(8, 3, 1, 3, 1, 0, 0, 12, l)}, {GHX_DT_F64}, {}, "not a multiple of the element size");
    refused({ok, entry(8, 3, 1, 4, 1, 0, 1, 0, m)}, {GHX_DT_F64, GHX_DT_F64}, {}, "differ in their data descriptor");
    refused({ok, entry(8, 2, 1, 3, 1, 0, 1, 0, m)}, {GHX_DT_F64, GHX_DT_F64}, {}, "differ in their data descriptor");
    refused({ok}, {GHX_DT_F64}, {entry(8, 3, 0, 3, 1, 0, 0, 0, m)}, "differ in their data descriptor");
    refused({ok, entry(8, 3, 1, 3, 1, 0, 1, 0, m)}, {GHX_DT_F64, GHX_DT_I64}, {}, "differ in their dtype");
    refused({ok}, {GHX_DT_F64}, {entry(8, 3, 1, 3, 1, 0, 0, 0, l)}, "is both a sum destination and a zero destination");
    // more records than 32 bits index: refused before a list is read (the lists hold 10 lids)
    ghx_upack_entry huge = ok, half = ok;
    huge.n_lids = int64_t(1) << 32;
    half.n_lids = int64_t(1) << 31;
    refused({huge}, {GHX_DT_F64}, {}, "more than 2^32 - 1 contribution records");
    refused({half, half}, {GHX_DT_F64, GHX_DT_F64}, {}, "more than 2^32 - 1 contribution records");
    huge.field_slot = 1;
    refused({ok}, {GHX_DT_F64}, {huge}, "more than 2^32 - 1 zero cells");
    ghx_upack_entry bad = ok;
    bad.lids = nullptr;
    refused({bad}, {GHX_DT_F64}, {}, "bad index list");
    bad = ok;
    bad.n_lids = -1;
    refused({bad}, {GHX_DT_F64}, {}, "bad index list");
    // overlapping buffer ranges are fine: contributions are only read
    const ghx_upack_entry two[2] = {ok, entry(8, 3, 1, 3, 1, 1, 0, 8, m)};
    const int32_t dt[2] = {GHX_DT_F64, GHX_DT_F64};
    ghx_uaccum* p = nullptr;
    CHECK(ghx_uaccum_create(two, dt, 2, nullptr, 0, &p) == GHX_OK && p);
    CHECK(ghx_uaccum_destroy(p) == GHX_OK);
    // null arguments
    CHECK(ghx_uaccum_create(nullptr, nullptr, 1, nullptr, 0, &p) == GHX_ERR_INVALID && p == nullptr);
    CHECK(ghx_uaccum_create(two, nullptr, 2, nullptr, 0, &p) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_create(two, dt, 2, nullptr, 1, &p) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_create(two, dt, -1, nullptr, 0, &p) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_create(two, dt, 2, nullptr, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_execute(nullptr, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uaccum_destroy(nullptr) == GHX_OK);
    // an empty plan has nothing to launch
    CHECK(ghx_uaccum_create(nullptr, nullptr, 0, nullptr, 0, &p) == GHX_OK && p);
    CHECK(ghx_uaccum_execute(p, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_OK);
    CHECK(ghx_uaccum_destroy(p) == GHX_OK);
}
}  // namespace

int main()
{
    tables();
    sixty_four_slots();
    refusals();
    std::printf("uaccum_host_check: OK\n");
    return 0;
}
