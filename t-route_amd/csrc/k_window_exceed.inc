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
// TILING: k_record_tile.inc's record_tile_walk, shared with k_window_summary (that file's head has the reasons, the LDS bank
// arithmetic and the alignment rule behind VEC).
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
// output i is the set's i-th row.  Any of the four outputs may be NULL.  Resource usage: profiles/r23_resource_usage.txt.
struct WexcOut {
    int32_t *steps_over;
    int32_t *first_step;
    int32_t *last_step;
    int32_t *longest_run;
};

template <class T, bool VEC, int COL, int KP>
__global__ void __launch_bounds__(kRecRows, 2)
k_window_exceed(const T *__restrict__ out, const int32_t *__restrict__ rowset_pos, const int32_t *__restrict__ row_of_pos,
                const T *__restrict__ th, WexcOut o, int64_t nrows, int32_t nsteps, int32_t K)
{
    static_assert(COL >= 0 && COL < 3 && (KP == 1 || KP == 2 || KP == 4), "a column of (q, v, d); 1, 2 or 4 padded levels");
    __shared__ RecVec<T> s_tile[kRecTileVecs];
    __shared__ int64_t s_src[kRecRows];               // element offset of the tile's rows in `out`, -1 beyond the last row
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kRecRows + lane;
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

    int32_t cnt[KP], first[KP], last[KP], best[KP], run[KP], t = 1;
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = first[k] = last[k] = best[k] = run[k] = 0;
    record_tile_walk<T, VEC>(
        out, s_tile, s_src, mine, nsteps, [](T, T, T) {},
        [&](T q, T v, T d) {
            const T x = COL == 0 ? q : COL == 1 ? v : d;
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
        });
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
