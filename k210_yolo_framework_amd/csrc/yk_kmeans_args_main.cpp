// Stand-alone driver of yk_kmeans.hip's host side for `make kmeans-san` (address + undefined-behaviour sanitizers): the workspace query
// and every refusal of yk_anchor_kmeans_f64.  All of them return before the first HIP call, so no device is needed.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "yolo_hip.h"

static char g_err[512];
void yk_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_failed = 0;
static void expect(int rc, int want, const char *needle, const char *what) {
    const bool ok = rc == want && (want == YK_OK || strstr(g_err, needle));
    printf("%-4s %s -> %d%s%s\n", ok ? "ok" : "FAIL", what, rc, want == YK_OK ? "" : ": ", want == YK_OK ? "" : g_err);
    g_failed += !ok;
    g_err[0] = 0;
}

int main() {
    size_t bytes = 0;
    expect(yk_anchor_kmeans_workspace_bytes(40000, 9, 256, &bytes), YK_OK, "", "workspace n=40000 k=9 R=256");
    if (bytes != (size_t)256 * 79 * 9 * 20) printf("FAIL %zu bytes\n", bytes), ++g_failed;
    expect(yk_anchor_kmeans_workspace_bytes(1ll << 24, 32, 4096, &bytes), YK_OK, "", "workspace at every limit");
    if (bytes != (size_t)4096 * 32768 * 32 * 20) printf("FAIL %zu bytes\n", bytes), ++g_failed;
    expect(yk_anchor_kmeans_workspace_bytes(1, 1, 1, &bytes), YK_OK, "", "workspace n=1 k=1 R=1");
    if (bytes != 20) printf("FAIL %zu bytes\n", bytes), ++g_failed;
    expect(yk_anchor_kmeans_workspace_bytes(0, 9, 1, &bytes), YK_ERR_ARG, "n = 0", "n = 0");
    expect(yk_anchor_kmeans_workspace_bytes((1ll << 24) + 1, 9, 1, &bytes), YK_ERR_ARG, "n = 16777217", "n = 2^24 + 1");
    expect(yk_anchor_kmeans_workspace_bytes(-(1ll << 62), 9, 1, &bytes), YK_ERR_ARG, "n = -", "n very negative");
    expect(yk_anchor_kmeans_workspace_bytes(100, 0, 1, &bytes), YK_ERR_ARG, "k = 0", "k = 0");
    expect(yk_anchor_kmeans_workspace_bytes(100, 33, 1, &bytes), YK_ERR_ARG, "k = 33", "k = 33");
    expect(yk_anchor_kmeans_workspace_bytes(100, 3, 0, &bytes), YK_ERR_ARG, "restarts = 0", "restarts = 0");
    expect(yk_anchor_kmeans_workspace_bytes(100, 3, 4097, &bytes), YK_ERR_ARG, "restarts = 4097", "restarts = 4097");
    expect(yk_anchor_kmeans_workspace_bytes(100, 3, 2, nullptr), YK_ERR_ARG, "bytes is NULL", "bytes = NULL");

    // never dereferenced on the host: any non-NULL, 16-byte aligned value will do
    alignas(16) static char buf[64];
    double *d = (double *)buf;
    int32_t *i = (int32_t *)buf;
    expect(yk_anchor_kmeans_f64(d, 100, d, 33, 2, 10, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "k = 33", "run k = 33");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 0, 10, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "restarts = 0", "run restarts = 0");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 0, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "iters = 0", "run iters = 0");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 1001, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "iters = 1001", "run iters = 1001");
    expect(yk_anchor_kmeans_f64(nullptr, 100, d, 3, 2, 10, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_wh is NULL", "run d_wh = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, nullptr, 3, 2, 10, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_init is NULL", "run d_init = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, nullptr, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_centroids is NULL", "run d_centroids = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, d, nullptr, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_counts is NULL", "run d_counts = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, d, i, nullptr, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_score is NULL", "run d_score = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, d, i, d, nullptr, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "d_empty is NULL", "run d_empty = NULL");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, d, i, d, i, nullptr, nullptr, 1 << 20, nullptr), YK_ERR_ARG, "d_work is NULL", "run d_work = NULL");
    expect(yk_anchor_kmeans_f64(d + 1, 100, d, 3, 2, 10, d, i, d, i, nullptr, buf, 1 << 20, nullptr), YK_ERR_ARG, "16-byte aligned", "run d_wh misaligned");
    expect(yk_anchor_kmeans_f64(d, 100, d, 3, 2, 10, d, i, d, i, nullptr, buf, 119, nullptr), YK_ERR_ARG, "work_bytes = 119: 120 needed", "run workspace one byte short");
    printf(g_failed ? "%d FAILED\n" : "all refusals as declared\n", g_failed);
    return g_failed != 0;
}
