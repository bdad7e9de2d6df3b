// ghx_cache.cpp — the plan caches of the per-call entry points (ghx_structured_pack/unpack,
// ghx_unstructured_pack/unpack, ghx_cs_unpack): plans keyed by content, least recently used
// out first, retired plans freed once the streams that ran them have passed.
#include <hip/hip_runtime.h>

#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "ghx_cubed_sphere.hpp"
#include "ghx_plan.hpp"

namespace ghx
{
namespace
{
// Plan caches of the per-call convenience entry points (ghx_structured_pack/unpack,
// ghx_unstructured_pack/unpack), like the reference's pattern container that outlives its
// exchanges (include/ghex/pattern_container.hpp:84-87). A hit is exact: the structured key IS
// the content (descriptor, iteration spaces, direction); the unstructured entry keeps a host
// copy of its index list and compares it in full on every hit, so a list mutated in place gets
// a fresh plan. Evicted or replaced plans are never freed under the lock with a device-wide
// synchronisation: they are retired and freed once every stream that executed them has passed
// the event recorded after its last execution there (plans executed inside a stream capture are
// kept: a graph may still reference their device tables).
template<typename Plan>
struct cached_plan
{
    struct use
    {
        hipStream_t stream;
        hipEvent_t done;  // recorded after the latest execution on `stream`
    };
    std::unique_ptr<Plan> plan;
    std::vector<char> content;  // unstructured: the index list bytes the plan was built from
    std::vector<use> uses;      // one record per stream that has executed the plan
    bool captured = false;
    bool idle() const
    {
        for (const auto& u : uses)
            if (hipEventQuery(u.done) != hipSuccess) return false;
        return true;
    }
    ~cached_plan()
    {
        for (auto& u : uses) (void)hipEventDestroy(u.done);
    }
};

template<typename Plan>
class plan_lru
{
    using entry = std::shared_ptr<cached_plan<Plan>>;
    std::mutex mtx_;
    std::list<std::string> lru_;
    std::unordered_map<std::string, std::pair<entry, std::list<std::string>::iterator>> map_;
    std::vector<entry> retired_;
    static constexpr size_t kCap = 256;

    void retire(entry e) { retired_.push_back(std::move(e)); }
    void reap()  // free retired plans nobody holds whose last execution has completed
    {
        std::vector<entry> keep;
        for (auto& e : retired_)
        {
            const bool idle = e.use_count() == 1 && !e->captured && e->idle();
            if (!idle) keep.push_back(std::move(e));
        }
        retired_.swap(keep);
    }

  public:
    // the cached entry for `key` if `same(entry)` holds, else the one `make()` builds
    template<typename Same, typename Make>
    entry get(const std::string& key, Same&& same, Make&& make)
    {
        {
            std::lock_guard<std::mutex> lk(mtx_);
            auto it = map_.find(key);
            if (it != map_.end() && same(*it->second.first))
            {
                lru_.splice(lru_.begin(), lru_, it->second.second);
                return it->second.first;
            }
        }
        entry fresh = make();  // plan construction (device upload) outside the lock
        std::lock_guard<std::mutex> lk(mtx_);
        reap();
        auto it = map_.find(key);
        if (it != map_.end())
        {
            retire(it->second.first);  // stale content (or built concurrently): replace
            lru_.erase(it->second.second);
            map_.erase(it);
        }
        if (map_.size() >= kCap)
        {
            auto old = map_.find(lru_.back());
            retire(old->second.first);
            map_.erase(old);
            lru_.pop_back();
        }
        lru_.push_front(key);
        map_.emplace(key, std::make_pair(fresh, lru_.begin()));
        return fresh;
    }

    // stream-ordered record of a use (no host synchronisation). One event per stream: a later
    // execution on the same stream is ordered after the earlier ones, so re-recording that
    // stream's event keeps covering them; an execution on another stream gets its own record,
    // so a plan used on streams A then B is freed only once BOTH have passed their last use.
    void used(cached_plan<Plan>& c, void* stream)
    {
        hipStream_t s = static_cast<hipStream_t>(stream);
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &st);
        std::lock_guard<std::mutex> lk(mtx_);
        if (st != hipStreamCaptureStatusNone)
        {
            c.captured = true;
            return;
        }
        for (auto& u : c.uses)
            if (u.stream == s)
            {
                if (hipEventRecord(u.done, s) != hipSuccess) c.captured = true;
                return;
            }
        // a new stream: drop the records of streams that have passed their last use (bounds
        // the list for callers that rotate through many streams)
        std::vector<typename cached_plan<Plan>::use> live;
        for (auto& u : c.uses)
        {
            if (hipEventQuery(u.done) == hipSuccess) (void)hipEventDestroy(u.done);
            else live.push_back(u);
        }
        c.uses.swap(live);
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
        {
            c.captured = true;  // cannot track it: never free it
            return;
        }
        if (hipEventRecord(e, s) != hipSuccess)
        {
            (void)hipEventDestroy(e);
            c.captured = true;
            return;
        }
        c.uses.push_back({s, e});
    }
};

plan_lru<splan>& cache()
{
    static plan_lru<splan> c;
    return c;
}

plan_lru<uplan>& ucache()
{
    static plan_lru<uplan> c;
    return c;
}

// ghx_cs_unpack's cached plan: the ordinary and the transformed part of one field's spaces
// (sp: the ordinary part once more as a pack plan, for ghx_cs_pack_rotated; x serves both ways)
struct cs_field_plan
{
    std::unique_ptr<splan> s, sp;
    std::unique_ptr<xplan> x;
};

plan_lru<cs_field_plan>& cs_cache()
{
    static plan_lru<cs_field_plan> c;
    return c;
}
}  // namespace

int run_structured(const ghx_field_desc& f, const ghx_box* boxes, int n, int dir, void* field,
                   void* buffer, void* stream)
{
    std::string key(reinterpret_cast<const char*>(&f), sizeof(f));
    key.append(reinterpret_cast<const char*>(boxes), sizeof(ghx_box) * size_t(n));
    key.push_back(char(dir));
    auto c = cache().get(
        key, [](const cached_plan<splan>&) { return true; },
        [&] {
            ghx_pack_entry e{};
            e.field = f;
            e.boxes = boxes;
            e.n_boxes = n;
            auto p = std::make_shared<cached_plan<splan>>();
            p->plan = std::make_unique<splan>(&e, 1, dir);
            return p;
        });
    void* fp[1] = {field};
    void* bp[1] = {buffer};
    const int rc = c->plan->execute(fp, 1, bp, 1, stream);
    cache().used(*c, stream);
    return rc;
}

namespace
{
std::shared_ptr<cached_plan<cs_field_plan>> cs_field_plan_of(const ghx_field_desc& f, const ghx_cs_item& cs,
                                                             const ghx_box* local, const ghx_box* global,
                                                             const int32_t* tiles, int n)
{
    std::string key(reinterpret_cast<const char*>(&f), sizeof(f));
    key.append(reinterpret_cast<const char*>(&cs), sizeof(cs));
    key.append(reinterpret_cast<const char*>(local), sizeof(ghx_box) * size_t(n));
    key.append(reinterpret_cast<const char*>(global), sizeof(ghx_box) * size_t(n));
    key.append(reinterpret_cast<const char*>(tiles), sizeof(int32_t) * size_t(n));
    return cs_cache().get(
        key, [](const cached_plan<cs_field_plan>&) { return true; },
        [&] {
            cs_recv_plan rp;
            uint64_t off = 0;
            for (int b = 0; b < n; ++b)
            {
                is_pair sp{};
                for (int k = 0; k < 3; ++k)
                {
                    sp.lf[k] = local[b].first[k];
                    sp.ll[k] = local[b].last[k];
                    sp.gf[k] = global[b].first[k];
                    sp.gl[k] = global[b].last[k];
                }
                uint64_t nb = 0;
                cs_plan_space(rp, f, cs, sp, tiles[b], 0, 0, off, &nb);
                off += nb;
            }
            auto p = std::make_shared<cached_plan<cs_field_plan>>();
            p->plan = std::make_unique<cs_field_plan>();
            if (!rp.segs.empty())
            {
                p->plan->sp = std::make_unique<splan>(rp.segs, rp.gf, rp.gb, rp.sbytes, 0);
                p->plan->s = std::make_unique<splan>(std::move(rp.segs), rp.gf, rp.gb, rp.sbytes, 1);
            }
            if (!rp.xs.empty()) p->plan->x = std::make_unique<xplan>(std::move(rp.xs));
            return p;
        });
}
}  // namespace

int run_cs_unpack(const ghx_field_desc& f, const ghx_cs_item& cs, const ghx_box* local,
                  const ghx_box* global, const int32_t* tiles, int n, void* field, void* buffer,
                  void* stream)
{
    auto c = cs_field_plan_of(f, cs, local, global, tiles, n);
    void* fp[1] = {field};
    void* bp[1] = {buffer};
    int rc = GHX_OK;
    if (c->plan->s) rc = c->plan->s->execute(fp, 1, bp, 1, stream);
    if (rc == GHX_OK && c->plan->x) rc = c->plan->x->execute(fp, 1, bp, 1, stream);
    cs_cache().used(*c, stream);
    return rc;
}

int run_cs_pack_rotated(const ghx_field_desc& f, const ghx_cs_item& cs, const ghx_box* local,
                        const ghx_box* global, const int32_t* tiles, int n, const void* field,
                        void* buffer, void* stream)
{
    auto c = cs_field_plan_of(f, cs, local, global, tiles, n);
    void* fp[1] = {const_cast<void*>(field)};
    void* bp[1] = {buffer};
    int rc = GHX_OK;
    if (c->plan->sp) rc = c->plan->sp->execute(fp, 1, bp, 1, stream);
    if (rc == GHX_OK && c->plan->x) rc = c->plan->x->execute_pack(fp, 1, bp, 1, stream);
    cs_cache().used(*c, stream);
    return rc;
}

int run_unstructured(const ghx_udata_desc& d, const void* lids, int32_t lid_bytes, int64_t n,
                     int dir, void* values, void* buffer, void* stream)
{
    std::string key(reinterpret_cast<const char*>(&d), sizeof(d));
    const uint64_t meta[4] = {uint64_t(reinterpret_cast<uintptr_t>(lids)), uint64_t(n),
                              uint64_t(lid_bytes), uint64_t(dir)};
    key.append(reinterpret_cast<const char*>(meta), sizeof(meta));
    const size_t nbytes = size_t(n) * size_t(lid_bytes);
    auto c = ucache().get(
        key,
        [&](const cached_plan<uplan>& e) {
            return e.content.size() == nbytes && std::memcmp(e.content.data(), lids, nbytes) == 0;
        },
        [&] {
            std::vector<int64_t> wide;
            const int64_t* l64 = static_cast<const int64_t*>(lids);
            if (lid_bytes == 4)
            {
                wide.resize(size_t(n));
                for (int64_t i = 0; i < n; ++i) wide[size_t(i)] = static_cast<const int32_t*>(lids)[i];
                l64 = wide.data();
            }
            ghx_upack_entry e{};
            e.data = d;
            e.lids = l64;
            e.n_lids = n;
            auto p = std::make_shared<cached_plan<uplan>>();
            p->plan = std::make_unique<uplan>(&e, 1, dir);
            p->content.assign(static_cast<const char*>(lids), static_cast<const char*>(lids) + nbytes);
            return p;
        });
    void* fp[1] = {values};
    void* bp[1] = {buffer};
    const int rc = c->plan->execute(fp, 1, bp, 1, stream);
    ucache().used(*c, stream);
    return rc;
}
}  // namespace ghx
