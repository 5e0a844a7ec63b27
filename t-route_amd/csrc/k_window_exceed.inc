// k_window_exceed -- one pass over a window's assembled result out[nseg][nsteps][3] = (q, v, d) per step, row-major, that leaves
// per output row i and level k < K, for ONE of the three quantities x = out[row][t][COL] against the row's threshold th[row][k]
// (trmc_plan_set_thresholds; trmc_window_exceedance, abi.inc), with over(t) := x[t] > th compared in T -- false when either side
// is a NaN, equality is not over:
//   steps_over   number of t in 1..nsteps with over(t)
//   first_step   the smallest such t (1-based), 0 if none
//   last_step    the largest such t, 0 if none
//   longest_run  length of the longest run of consecutive t with over(t), 0 if none
// all int32 [nrows][K], row-major.
//
// TILING: k_window_summary's (k_window_summary.inc, whose head has the reasons and the LDS bank arithmetic), kept as a copy here so
// that that kernel's compiled form cannot move.  A block of ONE wavefront owns kWexcRows = 64 rows and walks their records in chunks
// of kWexcSteps<T> = 128 / sizeof(T) steps: a row's chunk is 384 contiguous bytes.  The tile goes global -> registers as 24 16-byte
// vectors per lane (eight consecutive lanes on one 128-byte line of a row), from there to LDS with 16-byte stores at a row pitch
// of 400 B (conflict-free for the walk's ds_read_b128), and the next chunk's 24 loads are issued BEFORE the walk.  16-byte loads
// need every row's record 16-byte aligned (nsteps % (16 / sizeof(T)) == 0); any other nsteps goes element by element (VEC = false).
//
// WALK.  Lane r walks row r's chunk in step order.  All three columns of a step arrive in the lane's vectors, the one compared is a
// template parameter, so the other two cost nothing.  Per level five running ints -- count, first, last, longest, current run --
// carried from chunk to chunk in registers: 20 for KP = 4 beside the 96 VGPRs of staged vectors.  A step and level is five VALU
// instructions (compare, add, two selects, max, and the run's select).
// LEVELS.  KP in {1, 2, 4} is the width of the device table's rows, [nseg][KP] in T with +inf behind the plan's K levels (K = 3
// rides in KP = 4; +inf is never over): a row's thresholds are ONE load of KP elements (16 B for four fp32) before the walk.  The
// outputs hold exactly K columns: one vector store per lane and output where K == KP, K scalar stores otherwise.
//
// `rowset_pos` (NULL: output i = row i): plan positions of a registered set, row_of_pos takes them to rows of `out` and of `th`;
// output i is the set's i-th row.  Any of the four outputs may be NULL.  Resource usage: profiles/r20_resource_usage.txt.
constexpr int kWexcRows = 64;
template <class T> constexpr int kWexcSteps = 128 / (int)sizeof(T);
constexpr int kWexcChunkBytes = 384, kWexcPitchBytes = kWexcChunkBytes + 16;

struct WexcOut {
    int32_t *steps_over;
    int32_t *first_step;
    int32_t *last_step;
    int32_t *longest_run;
};

template <class T, bool VEC, int COL, int KP>
__global__ void __launch_bounds__(kWexcRows, 2)
k_window_exceed(const T *__restrict__ out, const int32_t *__restrict__ rowset_pos, const int32_t *__restrict__ row_of_pos,
                const T *__restrict__ th, WexcOut o, int64_t nrows, int32_t nsteps, int32_t K)
{
    static_assert(COL >= 0 && COL < 3 && (KP == 1 || KP == 2 || KP == 4), "a column of (q, v, d); 1, 2 or 4 padded levels");
    typedef T V __attribute__((ext_vector_type(16 / sizeof(T)))); // 16 bytes: float4 / double2
    constexpr int VE = 16 / (int)sizeof(T);           // elements of a vector = steps of a group of three vectors
    constexpr int C = kWexcSteps<T>;                  // steps of a chunk
    constexpr int CV = kWexcChunkBytes / 16;          // vectors of a row's chunk (24)
    constexpr int PV = kWexcPitchBytes / 16;          // LDS row pitch in vectors (25)
    constexpr int PE = kWexcPitchBytes / (int)sizeof(T), CE = 3 * C; // ... and in elements; elements of a row's chunk
    constexpr int NV = CV;                            // vectors a lane stages per chunk: 64 rows x 24 / 64 lanes
    __shared__ V s_tile[kWexcRows * PV];
    __shared__ int64_t s_src[kWexcRows];              // element offset of the tile's rows in `out`, -1 beyond the last row
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kWexcRows + lane;
    const bool mine = i < nrows;
    // the row's KP thresholds, one load (the table's rows are KP * sizeof(T) apart from a 256-byte-aligned base)
    T lim[KP];
    {
        int64_t row = -1;
        if (mine) row = rowset_pos ? (int64_t)row_of_pos[rowset_pos[i]] : i;
        s_src[lane] = row < 0 ? -1 : row * (int64_t)nsteps * 3;
        if constexpr (KP == 1) {
            lim[0] = row < 0 ? T(0) : th[row];
        } else {
            typedef T TV __attribute__((ext_vector_type(KP)));
            const TV x = *reinterpret_cast<const TV *>(th + (row < 0 ? 0 : row) * KP);
#pragma unroll
            for (int k = 0; k < KP; ++k) lim[k] = x[k];
        }
    }
    __syncthreads();
    T *const s_elem = reinterpret_cast<T *>(s_tile);

    // (VEC) lane -> the row groups and the 16-byte piece of a line it stages
    const int lr = lane >> 3, lc = lane & 7;
    V stage[VEC ? NV : 1];
    const T *base[VEC ? 8 : 1];
    if constexpr (VEC) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int64_t src = s_src[lr + 8 * b];
            base[b] = src >= 0 ? out + src + lc * VE : nullptr;
        }
    }
    // chunk [c0, c0 + cl): global -> registers (VEC) ...
    auto fetch = [&](int32_t c0, int32_t cl) {
        if constexpr (VEC) {
            const int nv = cl * 3 / VE; // (whole: see the head)
#pragma unroll
            for (int b = 0; b < 8; ++b)
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    // (beyond the last row or a short chunk's end: the result's first vector instead -- loaded, staged, never walked)
                    const T *const p = (base[b] && lc + 8 * m < nv) ? base[b] + (int64_t)c0 * 3 + m * 8 * VE : out;
                    stage[b * 3 + m] = *reinterpret_cast<const V *>(p);
                }
        }
    };
    // ... registers -> LDS (VEC), or global -> LDS element by element
    auto put = [&](int32_t c0, int32_t cl) {
        if constexpr (VEC) {
#pragma unroll
            for (int b = 0; b < 8; ++b)
#pragma unroll
                for (int m = 0; m < 3; ++m) s_tile[(lr + 8 * b) * PV + lc + 8 * m] = stage[b * 3 + m];
        } else {
            const int ne = cl * 3;
#pragma unroll 8
            for (int j = lane; j < kWexcRows * CE; j += kWexcRows) {
                const int r = j / CE, c = j - r * CE;
                const int64_t src = s_src[r];
                if (src >= 0 && c < ne) s_elem[r * PE + c] = out[src + (int64_t)c0 * 3 + c];
            }
        }
    };

    int32_t cnt[KP], first[KP], last[KP], best[KP], run[KP], t = 1;
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = first[k] = last[k] = best[k] = run[k] = 0;
    auto step = [&](T x) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool over = x > lim[k]; // (ordered compare: false when either side is a NaN)
            cnt[k] += over ? 1 : 0;
            first[k] = (over && first[k] == 0) ? t : first[k];
            last[k] = over ? t : last[k];
            run[k] = over ? run[k] + 1 : 0;
            best[k] = max(best[k], run[k]);
        }
        ++t;
    };

    fetch(0, min(C, nsteps));
    for (int32_t c0 = 0; c0 < nsteps; c0 += C) {
        const int32_t cl = min(C, nsteps - c0);
        put(c0, cl);
        __syncthreads();
        if (c0 + C < nsteps) fetch(c0 + C, min(C, nsteps - c0 - C));
        if (mine) {
            const V *const rv = s_tile + lane * PV;
            const T *const re = s_elem + lane * PE;
            int32_t g = 0;
#pragma unroll 2
            for (; g + VE <= cl; g += VE) {
                T e[3 * VE];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const V x = rv[g / VE * 3 + k];
#pragma unroll
                    for (int m = 0; m < VE; ++m) e[k * VE + m] = x[m];
                }
#pragma unroll
                for (int m = 0; m < VE; ++m) step(e[3 * m + COL]);
            }
            for (; g < cl; ++g) step(re[3 * g + COL]);
        }
        __syncthreads();
    }
    if (!mine) return;
    auto store = [&](int32_t *dst, const int32_t (&v)[KP]) {
        if (!dst) return;
        if constexpr (KP > 1) {
            if (K == KP) { // [nrows][KP] from a 256-byte-aligned column: the lane's KP ints are one aligned vector
                typedef int32_t IV __attribute__((ext_vector_type(KP)));
                IV x;
#pragma unroll
                for (int k = 0; k < KP; ++k) x[k] = v[k];
                *reinterpret_cast<IV *>(dst + i * KP) = x;
                return;
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) dst[i * K + k] = v[k];
    };
    store(o.steps_over, cnt);
    store(o.first_step, first);
    store(o.last_step, last);
    store(o.longest_run, best);
}
