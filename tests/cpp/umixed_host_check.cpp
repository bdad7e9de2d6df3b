// umixed_host_check — stand-alone host program (its own main; links the library's sources) for
// the index-list pack that also completes the self messages: ghx_umixed_create / _info /
// _peer_segment with ghx_uself_info / _segment / _destroy through the C header, created without a
// device. A plan with self and peer messages of every row form and table width, its counts and
// peer segments against ghx_uself_create's plan of the self part and ghx_uplan_create's pack plan
// of the peer part, a peer list split below 2^30 bytes; every additional refusal with its reason,
// the self part's refusals passed through; indices out of range and null arguments. Built with
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

// peer segment k of the mixed plan equals segment k of the pack plan of the same entries
void same_peer_segments(const ghx_uself* p, const ghx_upack_entry* peers, int n_peers)
{
    ghx_uplan* u = nullptr;
    CHECK(ghx_uplan_create(peers, n_peers, 0, &u) == GHX_OK && u);
    uint64_t bytes = 0;
    int32_t ns = -1, nt = -1, st = -1, ps = -1, pt = -1;
    CHECK(ghx_uplan_info(u, &bytes, &ns, &nt) == GHX_OK);
    CHECK(ghx_umixed_info(p, &st, &ps, &pt) == GHX_OK);
    CHECK(ps == ns && pt == nt && st > 0);
    for (int k = 0; k < ns; ++k)
    {
        ghx_usegment_info a, b;
        CHECK(ghx_umixed_peer_segment(p, k, &a) == GHX_OK);
        CHECK(ghx_uplan_segment(u, k, &b) == GHX_OK);
        CHECK(a.field_off == b.field_off && a.buf_off == b.buf_off && a.bytes == b.bytes);
        CHECK(a.index_stride_b == b.index_stride_b && a.level_stride_b == b.level_stride_b);
        CHECK(a.row_bytes == b.row_bytes && a.tile_bytes == b.tile_bytes && a.n == b.n);
        CHECK(a.field_slot == b.field_slot && a.buffer_slot == b.buffer_slot);
        CHECK(a.mode == b.mode && a.wlog2 == b.wlog2 && a.lid64 == b.lid64 && a.runs == b.runs);
        CHECK(a.bytes <= (1u << 30));
    }
    ghx_usegment_info s;
    CHECK(ghx_umixed_peer_segment(p, ns, &s) == GHX_ERR_INVALID);
    CHECK(ghx_umixed_peer_segment(p, -1, &s) == GHX_ERR_INVALID);
    CHECK(ghx_umixed_peer_segment(p, 0, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_umixed_peer_segment(nullptr, 0, &s) == GHX_ERR_INVALID);
    CHECK(ghx_uplan_destroy(u) == GHX_OK);
}

void every_form()
{
    const int64_t big = (int64_t(1) << 31) + 5;
    const auto s0 = some_lids(3001, 0, 0), t0 = some_lids(3001, 5000, 0);
    const auto s1 = some_lids(3002, 0, 0), t1 = some_lids(3002, 5000, big);
    const auto p0 = some_lids(1031, 100, 0), p1 = some_lids(257, 0, big), p2 = some_lids(5, 9000, 0);
    const ghx_upack_entry src[2] = {
        entry(8, 3, 1, 4, 1, 0, 0, 0, s0),  // mode 0: 24-B rows, padded source
        entry(4, 3, 1, 3, 1, 1, 1, 8, s1),  // contiguous against strided levels: mode 1
    };
    const ghx_upack_entry dst[2] = {
        entry(8, 3, 1, 3, 1, 4, 0, 0, t0),
        entry(4, 3, 1, 1, 10007, 5, 1, 8, t1),
    };
    const ghx_upack_entry peers[3] = {
        entry(16, 3, 0, 1, 10010, 0, 2, 20, p0),             // mode 2, offset 20 narrows 16-B elements
        entry(4, 1, 1, 1, 1, 2, 2, 1031 * 48 + 32, p1),      // run-eligible, int64 table, after a pad gap
        entry(8, 2, 1, 2, 1, 4, 0, 3001 * 24 + 16, p2),      // reads a receiving field, shares buffer 0
    };
    ghx_uself *p = nullptr, *q = nullptr;
    CHECK(ghx_umixed_create(src, dst, 2, peers, 3, &p) == GHX_OK && p);
    CHECK(ghx_uself_create(src, dst, 2, &q) == GHX_OK && q);
    uint64_t bytes = 0, sbytes = 0;
    int32_t ns = -1, nt = -1, sns = -1, snt = -1, st = -1, ps = -1, pt = -1;
    CHECK(ghx_uself_info(p, &bytes, &ns, &nt) == GHX_OK);
    CHECK(ghx_uself_info(q, &sbytes, &sns, &snt) == GHX_OK);
    CHECK(ghx_umixed_info(p, &st, &ps, &pt) == GHX_OK);
    CHECK(sns == 2 && ps == 3 && ns == sns + ps && st == snt && nt == snt + pt);
    CHECK(bytes == sbytes + 1031u * 48 + 257u * 4 + 5u * 16);
    // a plan of ghx_uself_create: all self tiles, no peer part
    CHECK(ghx_umixed_info(q, &st, &ps, &pt) == GHX_OK && st == snt && ps == 0 && pt == 0);
    ghx_usegment_info none;
    CHECK(ghx_umixed_peer_segment(q, 0, &none) == GHX_ERR_INVALID);
    CHECK(ghx_umixed_info(nullptr, &st, &ps, &pt) == GHX_ERR_INVALID);
    CHECK(ghx_umixed_info(p, nullptr, nullptr, nullptr) == GHX_OK);
    // the self segments are the self plan's
    for (int k = 0; k < sns; ++k)
    {
        ghx_uself_segment_info a, b;
        CHECK(ghx_uself_segment(p, k, &a) == GHX_OK && ghx_uself_segment(q, k, &b) == GHX_OK);
        CHECK(a.mode == b.mode && a.wlog2 == b.wlog2 && a.row_bytes == b.row_bytes && a.bytes == b.bytes);
        CHECK(a.tile_bytes == b.tile_bytes && a.buf_slot == b.buf_slot && a.buf_off == b.buf_off);
        CHECK(a.src_lid64 == b.src_lid64 && a.dst_lid64 == b.dst_lid64 && a.message == k);
    }
    ghx_uself_segment_info s;
    CHECK(ghx_uself_segment(p, sns, &s) == GHX_ERR_INVALID);
    same_peer_segments(p, peers, 3);
    // too few pointers: refused before anything is launched
    void* one[1] = {reinterpret_cast<void*>(4096)};
    CHECK(ghx_uself_execute(p, one, 1, one, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
    CHECK(ghx_uself_destroy(q) == GHX_OK);
}

// a levels-last peer list of more than 2^30 bytes: split level by level as the pack plan splits it
void split_list()
{
    const int64_t n = (int64_t(1) << 20) + 3;  // x 1 KiB x 2 levels > 2^30: two pieces per level
    std::vector<int64_t> l(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) l[size_t(i)] = n - 1 - i;
    const auto s = some_lids(300, 0, 0), t = some_lids(300, 5000, 0);
    const ghx_upack_entry se = entry(8, 1, 1, 1, 1, 0, 0, 0, s), de = entry(8, 1, 1, 1, 1, 1, 0, 0, t);
    const ghx_upack_entry pe = entry(1024, 2, 0, 1, n + 1, 2, 1, 256, l);
    ghx_uself* p = nullptr;
    CHECK(ghx_umixed_create(&se, &de, 1, &pe, 1, &p) == GHX_OK);
    int32_t ps = -1;
    CHECK(ghx_umixed_info(p, nullptr, &ps, nullptr) == GHX_OK && ps == 4);
    same_peer_segments(p, &pe, 1);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
}

void refused(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n, const ghx_upack_entry* peers,
             int np, const char* why)
{
    ghx_uself* p = reinterpret_cast<ghx_uself*>(8);
    CHECK(ghx_umixed_create(src, dst, n, peers, np, &p) == GHX_ERR_INVALID);
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
    const auto q = some_lids(40, 400, 0), r = some_lids(17, 800, 0);
    const ghx_upack_entry se = entry(8, 1, 1, 1, 1, 0, 0, 64, s), de = entry(8, 1, 1, 1, 1, 1, 0, 64, t);
    const ghx_upack_entry ok = entry(8, 1, 1, 1, 1, 0, 1, 0, q);
    refused(nullptr, nullptr, 0, &ok, 1, "no self message");
    refused(&se, &de, 1, nullptr, 0, "no peer message");
    refused(&se, &de, 1, nullptr, 1, "no peer message");
    auto peer = [&](const ghx_upack_entry& pe, const char* why) { refused(&se, &de, 1, &pe, 1, why); };
    const char* limit = "peer message's field or buffer slot is 64 or more";
    peer(entry(8, 1, 1, 1, 1, 64, 1, 0, q), limit);
    peer(entry(8, 1, 1, 1, 1, 0, 64, 0, q), limit);
    peer(entry(8, 1, 1, 1, 1, -1, 1, 0, q), "negative slot");
    peer(entry(8, 1, 1, 1, 1, 0, -1, 0, q), "negative slot");
    const char* over = "a peer message overlaps another message in one buffer";
    peer(entry(8, 1, 1, 1, 1, 0, 0, 0, q), over);               // 320 bytes from 0 into the self range
    peer(entry(8, 1, 1, 1, 1, 0, 0, 64 + 2399, r), over);       // the self range's last byte
    {
        const ghx_upack_entry two[2] = {entry(8, 1, 1, 1, 1, 0, 1, 0, q), entry(8, 1, 1, 1, 1, 0, 1, 312, r)};
        refused(&se, &de, 1, two, 2, over);
    }
    auto hit = q;
    hit[9] = t[250];
    peer(entry(8, 1, 1, 1, 1, 1, 1, 0, hit), "target cell of a self message is a source cell of a peer message");
    auto neg = q;
    neg[3] = -1;
    peer(entry(8, 1, 1, 1, 1, 0, 1, 0, neg), "negative local index");
    peer(entry(0, 1, 1, 1, 1, 0, 1, 0, q), "bad unstructured data descriptor");
    // the self part's refusals pass through
    {
        const ghx_upack_entry bad = entry(8, 1, 1, 1, 1, 1, 0, 64, u);
        refused(&se, &bad, 1, &ok, 1, "do not describe the same message bytes");
        auto both = t;
        both[9] = s[250];
        const ghx_upack_entry d2 = entry(8, 1, 1, 1, 1, 0, 0, 64, both);
        refused(&se, &d2, 1, &ok, 1, "both a source and a target");
        const ghx_upack_entry s64 = entry(8, 1, 1, 1, 1, 64, 0, 64, s);
        refused(&s64, &de, 1, &ok, 1, "at most 64 field and 64 buffer slots");
    }
    // accepted: the same lid on another field slot, a range that ends where the self range begins
    ghx_uself* p = nullptr;
    const ghx_upack_entry other = entry(8, 1, 1, 1, 1, 0, 1, 0, hit);
    CHECK(ghx_umixed_create(&se, &de, 1, &other, 1, &p) == GHX_OK);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
    const auto eight = some_lids(8, 900, 0);
    const ghx_upack_entry before = entry(8, 1, 1, 1, 1, 0, 0, 0, eight);
    CHECK(ghx_umixed_create(&se, &de, 1, &before, 1, &p) == GHX_OK);
    CHECK(ghx_uself_destroy(p) == GHX_OK);
    CHECK(ghx_umixed_create(&se, &de, 1, &ok, 1, nullptr) == GHX_ERR_INVALID);
}
}  // namespace

int main()
{
    every_form();
    split_list();
    refusals();
    std::printf("umixed_host_check: ok\n");
    return 0;
}
