// yk_lap.h — motmetrics.lap on the device, once: Jonker-Volgenant shortest augmenting paths in Crouse's form with the rule's stated order
// of operations and tie rules (k210_yolo_framework_amd/motmetrics.py), one problem by one wavefront, lanes owning columns.
// Two units include it and differ only in where a cost comes from: yk_mot.hip reads it from a matrix (lap_matrix_cost: yk_lap_f64 and
// the scores), yk_track.hip recomputes it from two LDS-resident boxes (track_pair_cost: assign = lap).
//
// A cost source is
//     cost.row(i)   called once per step of the search, for the row the step relaxes against; what it returns keeps that row's share of
//                   the work (a row pointer, a box) in registers for the sweep
//     row(j)        the double cost of column j in that row.
//
// Both including units are compiled with -ffp-contract=off and without packed fp32: one rounding per operation, as the rule's float64 steps.
// Must be called by a workgroup that is exactly ONE wavefront (64 threads).
#pragma once
#include "yk_common.h"

struct lap_lds {
    double *v, *dist, *u;                 // [n] column duals, [n] tentative distances, [m] row duals
    int *pred, *row4col, *scanned;        // [n] each
    int *col4row;                         // [m]
};

__host__ __device__ static inline size_t lap_vector_bytes(int m, int n) {
    return (size_t)YK_LAP_LDS_PER_COL * n + (size_t)YK_LAP_LDS_PER_ROW * m;
}

// does the cost matrix of a rows x cols problem live in LDS beside the vectors?  A function of the shape alone.
__host__ __device__ static inline bool yk_lap_resident(int rows, int cols) {
    const int m = rows < cols ? rows : cols, n = rows < cols ? cols : rows;
    return lap_vector_bytes(m, n) + (size_t)m * n * sizeof(double) <= (size_t)YK_LAP_LDS_BYTES;
}

// v[n], dist[n], u[m], pred[n], row4col[n], scanned[n], col4row[m] from base (8-byte aligned); ends lap_vector_bytes(m, n) behind it
__device__ __forceinline__ lap_lds lap_carve(void *base, int m, int n) {
    lap_lds L;
    L.v = reinterpret_cast<double *>(base);
    L.dist = L.v + n;
    L.u = L.dist + n;
    L.pred = reinterpret_cast<int *>(L.u + m);
    L.row4col = L.pred + n;
    L.scanned = L.row4col + n;
    L.col4row = L.scanned + n;
    return L;
}

// the answer of a problem the wave solved transposed (tall) or as it stood: the wave's column of every row of the PROBLEM, or -1
__device__ __forceinline__ const int *lap_answer(const lap_lds &L, bool tall) { return tall ? L.row4col : L.col4row; }

// arg-min over (value asc, column asc) across the wave; col < 0 means "no candidate"
__device__ __forceinline__ void lap_wave_argmin(double &best, int &col) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oc = __shfl_xor(col, o, 64);
        if (oc >= 0 && (col < 0 || ob < best || (ob == best && oc < col))) {
            best = ob;
            col = oc;
        }
    }
}

// One problem by one wavefront: row i of the m the wave augments against column j of the n it searches (m <= n), the cost of the pair from
// `cost` (above).  Leaves col4row [m] and row4col [n] in L; the caller reads them after it.
template <class Cost>
__device__ void yk_lap_wave(const Cost &cost, int m, int n, const lap_lds &L, int lane) {
    for (int j = lane; j < n; j += 64) {
        L.v[j] = 0.0;
        L.row4col[j] = -1;
    }
    for (int i = lane; i < m; i += 64) {
        L.u[i] = 0.0;
        L.col4row[i] = -1;
    }
    __syncthreads();
    for (int cur = 0; cur < m; ++cur) {
        for (int j = lane; j < n; j += 64) {
            L.dist[j] = INFINITY;
            L.pred[j] = -1;
            L.scanned[j] = 0;
        }
        double minval = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            const double ui = L.u[i];
            const auto row = cost.row(i);
            double best = INFINITY;
            int bcol = -1;
            for (int j = lane; j < n; j += 64) {
                if (L.scanned[j]) continue;
                const double r = ((minval + row(j)) - ui) - L.v[j];
                double d = L.dist[j];
                if (r < d) {
                    d = r;
                    L.dist[j] = r;
                    L.pred[j] = i;
                }
                if (bcol < 0 || d < best) {
                    best = d;
                    bcol = j;
                }
            }
            lap_wave_argmin(best, bcol);                                 // (an unscanned column exists while no sink was found: m <= n)
            minval = best;
            if ((bcol & 63) == lane) L.scanned[bcol] = 1;
            const int holder = L.row4col[bcol];
            if (holder < 0) sink = bcol;
            else i = holder;
        }
        __syncthreads();
        // the duals: every scanned column but the sink is held by a row of its own, so no two lanes write one u
        for (int j = lane; j < n; j += 64) {
            if (!L.scanned[j]) continue;
            const double t = minval - L.dist[j];
            L.v[j] = L.v[j] - t;
            if (j != sink) {
                const int r = L.row4col[j];
                L.u[r] = L.u[r] + t;
            }
        }
        __syncthreads();
        if (lane == 0) {
            L.u[cur] = L.u[cur] + minval;
            int j = sink;
            for (;;) {
                const int r = L.pred[j];
                L.row4col[j] = r;
                const int next = L.col4row[r];
                L.col4row[r] = j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
}
