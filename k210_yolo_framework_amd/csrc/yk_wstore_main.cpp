// yk_wstore_main.cpp — the weight store's host logic (yk_wstore.h) on its own, behind a host-memory "device": insert, hit, a hash
// collision between different bytes, keys that differ in one field, the last release, a failed upload, a packer that throws and
// concurrent inserts.  Built with the address and undefined-behaviour sanitizers and run on the CPU (`make wstore-san`); never loaded
// into python.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <new>
#include <thread>

#include "yk_wstore.h"

static std::atomic<long> g_live{0}, g_uploads{0}, g_packs{0};
static bool g_fail = false;

static void *fake_upload(void *, int, const void *src, size_t bytes) {
    if (g_fail) return nullptr;
    void *d = malloc(bytes ? bytes : 1);
    memcpy(d, src, bytes);
    ++g_live;
    ++g_uploads;
    return d;
}
static void fake_release(void *, int, void *d) {
    free(d);
    --g_live;
}
static uint64_t constant_hash(const yk_wsrc *, int) { return 42; }

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

// the "packer": every source float doubled; aux = {their sum}
static yk_wpack_fn doubler(const std::vector<float> &w) {
    return [&w](std::vector<uint8_t> &out, std::vector<float> &aux) {
        ++g_packs;
        std::vector<float> v(w.size());
        float s = 0.f;
        for (size_t i = 0; i < w.size(); ++i) {
            v[i] = 2.f * w[i];
            s += w[i];
        }
        out.resize(v.size() * sizeof(float));
        memcpy(out.data(), v.data(), out.size());
        aux = {s};
    };
}
static yk_went *get(yk_wstore &st, int device, int tag, int32_t par, const std::vector<float> &w) {
    const yk_wsrc src{w.data(), w.size() * sizeof(float)};
    return st.acquire(device, tag, &par, 1, &src, 1, doubler(w));
}

static int run(uint64_t (*hash)(const yk_wsrc *, int)) {
    yk_wstore st({nullptr, fake_upload, fake_release}, hash);
    std::vector<float> a(1000), b(1000);
    for (int i = 0; i < 1000; ++i) a[i] = b[i] = 0.25f * (float)i;
    b[999] += 1.f;                                                   // one element differs
    const long packs0 = g_packs;

    yk_went *e1 = get(st, 0, 1, 7, a);                               // insert
    CHECK(e1 && st.entries() == 1 && g_packs == packs0 + 1 && e1->bytes == 4000 && e1->aux.size() == 1);
    CHECK(((const float *)e1->d)[999] == 2.f * a[999]);
    yk_went *e2 = get(st, 0, 1, 7, a);                               // hit: same entry, nothing packed
    CHECK(e2 == e1 && st.entries() == 1 && g_packs == packs0 + 1 && st.hits() == 1);
    std::vector<float> a_copy(a);                                    // ... also from another address
    CHECK(get(st, 0, 1, 7, a_copy) == e1 && e1->refs == 3);
    yk_went *eb = get(st, 0, 1, 7, b);                               // other bytes (the same hash under constant_hash): its own entry
    CHECK(eb && eb != e1 && st.entries() == 2 && ((const float *)eb->d)[999] == 2.f * b[999]);
    yk_went *ed = get(st, 1, 1, 7, a), *et = get(st, 0, 2, 7, a), *ep = get(st, 0, 1, 8, a);   // other device / packer / parameter
    CHECK(ed && et && ep && ed != e1 && et != e1 && ep != e1 && ed != et && et != ep && st.entries() == 5);
    std::vector<float> shorter(a.begin(), a.end() - 1);              // a prefix is not a match
    yk_went *es = get(st, 0, 1, 7, shorter);
    CHECK(es && es != e1 && st.entries() == 6);
    {   // two ranges [x | y] are not the one range [xy]
        const yk_wsrc two[2] = {{a.data(), 2000}, {(const uint8_t *)a.data() + 2000, 2000}};
        const int32_t par = 7;
        yk_went *e = st.acquire(0, 1, &par, 1, two, 2, doubler(a));
        CHECK(e && e != e1 && st.entries() == 7);
        st.release(e);
        CHECK(st.entries() == 6);
    }
    g_fail = true;                                                   // a failed upload inserts nothing
    std::vector<float> c(10, 3.f);
    CHECK(get(st, 0, 1, 7, c) == nullptr && st.entries() == 6);
    g_fail = false;
    {   // nor does a packer that throws; the half-made entry is freed (the leak check of the address sanitizer sees it otherwise)
        const yk_wsrc src{c.data(), c.size() * sizeof(float)};
        const int32_t par = 7;
        bool thrown = false;
        try {
            st.acquire(0, 1, &par, 1, &src, 1, [](std::vector<uint8_t> &, std::vector<float> &) { throw std::bad_alloc(); });
        } catch (const std::bad_alloc &) {
            thrown = true;
        }
        CHECK(thrown && st.entries() == 6);
        yk_went *e = get(st, 0, 1, 7, c);                            // the store is not left locked, and the key still works
        CHECK(e && st.entries() == 7);
        st.release(e);
    }

    st.release(es); st.release(ep); st.release(et); st.release(ed); st.release(eb);
    CHECK(st.entries() == 1 && g_live == 1);
    st.release(e1); st.release(e1);
    CHECK(st.entries() == 1 && e1->refs == 1);
    st.release(e1);                                                  // the last one frees the device buffer and the host copy
    CHECK(st.entries() == 0 && g_live == 0);
    yk_went *e3 = get(st, 0, 1, 7, a);                               // and the next plan builds it again
    CHECK(e3 && st.entries() == 1 && g_live == 1 && g_packs > packs0 + 1);
    st.release(e3);
    CHECK(st.entries() == 0 && g_live == 0);

    // eight threads, the same two keys, acquire / release in a loop and a final acquire each: two entries, packed once per lifetime
    std::vector<yk_went *> got(16, nullptr);
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([&, t] {
            for (int k = 0; k < 50; ++k) {
                yk_went *x = get(st, 0, 1, 7, a), *y = get(st, 0, 1, 7, b);
                st.release(x);
                st.release(y);
            }
            got[2 * t] = get(st, 0, 1, 7, a);
            got[2 * t + 1] = get(st, 0, 1, 7, b);
        });
    for (auto &t : th) t.join();
    CHECK(st.entries() == 2 && g_live == 2);
    for (int t = 0; t < 8; ++t) CHECK(got[2 * t] == got[0] && got[2 * t + 1] == got[1] && got[0] != got[1]);
    CHECK(got[0]->refs == 8 && got[1]->refs == 8);
    for (yk_went *e : got) st.release(e);
    CHECK(st.entries() == 0 && g_live == 0);
    return 0;
}

int main() {
    if (run(yk_wstore_hash)) return 1;
    if (run(constant_hash)) return 1;                                // every lookup is a hash collision: the byte compare decides
    const std::vector<float> x(3, 1.f), y(3, 2.f);
    const yk_wsrc sx{x.data(), 12}, sy{y.data(), 12}, sx2{x.data(), 8};
    if (yk_wstore_hash(&sx, 1) == yk_wstore_hash(&sy, 1) || yk_wstore_hash(&sx, 1) == yk_wstore_hash(&sx2, 1)) return 1;
    printf("yk_wstore: ok (%ld uploads)\n", g_uploads.load());
    return 0;
}
