// yk_wstore.h — the store of packed, immutable plan buffers (conv weight tiles, folded BatchNorm tables, depthwise parameter tables):
// plans that pack the same source values the same way for the same device read ONE device copy.  Host code only and free of HIP: the
// device side is the three-function interface below, so the key / hash / reference-count logic also builds into a program of its own
// (yk_wstore_main.cpp, `make wstore-san`).
//
// An entry is keyed by everything that determines its packed bytes: the device, a tag naming the packer, the packer's integer parameters
// (tile order, channel padding, slab count, ...) and the source values - their length, a 64-bit hash, and on a hash hit a byte compare
// with the copy of the source the entry keeps: a hash hit alone never aliases two models.  Besides the device buffer an entry keeps the
// few floats its packer derived on the host (gains, offsets, the weight exponent), so a hit skips the host-side packing altogether.
// acquire() takes a reference, release() drops it, the last release frees the device buffer and the host copy.  One mutex guards the
// store; it is held while a missing entry is packed and uploaded, so plans created at the same time still make one entry.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

struct yk_wstore_dev {
    void *ctx;
    void *(*upload)(void *ctx, int device, const void *src, size_t bytes);   // a new device buffer holding src[0, bytes); nullptr = failed
    void (*release)(void *ctx, int device, void *d);
};

struct yk_wsrc {   // one range of source values
    const void *p;
    size_t bytes;
};

struct yk_went {
    int device = 0, tag = 0;
    std::vector<int32_t> par;
    std::vector<size_t> src_len;     // the length of every source range ...
    std::vector<uint8_t> src;        // ... and their bytes, one after the other
    uint64_t hash = 0;
    void *d = nullptr;
    size_t bytes = 0;
    std::vector<float> aux;
    long refs = 0;
};

// fills the packed bytes and the derived floats of a missing entry
using yk_wpack_fn = std::function<void(std::vector<uint8_t> &packed, std::vector<float> &aux)>;

static inline uint64_t yk_wstore_hash(const yk_wsrc *src, int nsrc) {   // 64-bit multiply-xorshift over 8-byte words, lengths included
    uint64_t h = 0x9e3779b97f4a7c15ull;
    auto mix = [&h](uint64_t v) {
        h = (h ^ v) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    };
    for (int s = 0; s < nsrc; ++s) {
        const uint8_t *b = (const uint8_t *)src[s].p;
        size_t n = src[s].bytes;
        mix((uint64_t)n);
        for (; n >= 8; n -= 8, b += 8) {
            uint64_t v;
            memcpy(&v, b, 8);
            mix(v);
        }
        if (n) {
            uint64_t v = 0;
            memcpy(&v, b, n);
            mix(v);
        }
    }
    return h;
}

class yk_wstore {
public:
    explicit yk_wstore(yk_wstore_dev dev, uint64_t (*hash)(const yk_wsrc *, int) = yk_wstore_hash) : dev_(dev), hash_(hash) {}
    ~yk_wstore() {
        for (auto &kv : map_) {   // (entries still referenced at exit: the process is going away, the device memory with it)
            delete kv.second;
        }
    }

    // the entry of (device, tag, par, source values), with one more reference; a missing one is packed, uploaded and inserted first.
    // nullptr: the upload failed (nothing was inserted).
    yk_went *acquire(int device, int tag, const int32_t *par, int npar, const yk_wsrc *src, int nsrc, const yk_wpack_fn &pack) {
        const uint64_t h = hash_(src, nsrc);
        std::lock_guard<std::mutex> lock(mu_);
        auto range = map_.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (same(*it->second, device, tag, par, npar, src, nsrc)) {
                ++it->second->refs;
                ++hits_;
                return it->second;
            }
        std::unique_ptr<yk_went> e(new yk_went());   // (pack may throw: nothing is inserted then, and nothing is left behind)
        e->device = device;
        e->tag = tag;
        e->par.assign(par, par + npar);
        e->hash = h;
        for (int s = 0; s < nsrc; ++s) {
            e->src_len.push_back(src[s].bytes);
            e->src.insert(e->src.end(), (const uint8_t *)src[s].p, (const uint8_t *)src[s].p + src[s].bytes);
        }
        std::vector<uint8_t> packed;
        pack(packed, e->aux);
        e->bytes = packed.size();
        e->d = dev_.upload(dev_.ctx, device, packed.data(), packed.size());
        if (!e->d) return nullptr;
        e->refs = 1;
        map_.emplace(h, e.get());
        return e.release();
    }

    void release(yk_went *e) {
        if (!e) return;
        std::lock_guard<std::mutex> lock(mu_);
        if (--e->refs > 0) return;
        auto range = map_.equal_range(e->hash);
        for (auto it = range.first; it != range.second; ++it)
            if (it->second == e) {
                map_.erase(it);
                break;
            }
        dev_.release(dev_.ctx, e->device, e->d);
        delete e;
    }

    size_t entries() {
        std::lock_guard<std::mutex> lock(mu_);
        return map_.size();
    }
    size_t hits() {
        std::lock_guard<std::mutex> lock(mu_);
        return hits_;
    }

private:
    static bool same(const yk_went &e, int device, int tag, const int32_t *par, int npar, const yk_wsrc *src, int nsrc) {
        if (e.device != device || e.tag != tag || (int)e.par.size() != npar || (int)e.src_len.size() != nsrc) return false;
        if (npar && memcmp(e.par.data(), par, sizeof(int32_t) * npar) != 0) return false;
        size_t at = 0;
        for (int s = 0; s < nsrc; ++s) {
            if (e.src_len[s] != src[s].bytes) return false;
            if (src[s].bytes && memcmp(e.src.data() + at, src[s].p, src[s].bytes) != 0) return false;
            at += src[s].bytes;
        }
        return true;
    }

    yk_wstore_dev dev_;
    uint64_t (*hash_)(const yk_wsrc *, int);
    std::mutex mu_;
    std::unordered_multimap<uint64_t, yk_went *> map_;
    size_t hits_ = 0;
};
