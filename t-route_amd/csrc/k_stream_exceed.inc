// k_stream_exceed -- THRESHOLD EXCEEDANCE OVER A WHOLE STREAM OF DAYS (trmc_stream_set_exceedance, trmc_stream_exceedance; launched
// by stream_complete_day, stream.inc, beside k_stream_summary).  The definition is the window kernel's (k_window_exceed.inc):
// over(t) := q[t] > th[row][k], compared in T -- false when either side is a NaN, equality is not over -- and per row and level
//   steps_over   number of steps t of the stream with over(t)
//   first_step   the smallest such t, 0 if none
//   last_step    the largest such t, 0 if none
//   longest_run  length of the longest run of consecutive t with over(t), 0 if none
// with t counted on over the days, 1-based from the stream's first step.  It is NOT a product of the day: a run that is open at a
// day's last step goes on at the next day's first, so the state -- those four and the current run -- lives in an accumulator
// outside the ring, as the totals of k_stream_total do, and this kernel folds one day into it, in day order.
//
// WALK: k_stream_summary's.  The day's flows are the time rows 1..nsteps of its slot's time-major plane; one thread per plan
// position walks them, so a wavefront reads 64 consecutive flows of a time row per load, and kStreamExceedUnroll independent
// loads are issued before the first compare that depends on them.  The row's KP thresholds are ONE load through row_of_pos (the
// plan's table: [nseg][KP] in row order, KP in {1, 2, 4}, +inf -- never over -- behind the K levels asked for).
// STATE: int32 acc[5][KP][nseg_pad] in PLAN order -- count, first, last, longest, current run -- so that a wavefront's reads and
// writes of it are whole lines, once per day; a step and level is the window kernel's five VALU instructions on 32-bit registers,
// which is why the state is 32 bits wide: at four levels the walk issues about as many VALU cycles as the plane's bytes take to
// arrive.  trmc_stream_push_day refuses the day that would take the stream's step count past INT32_MAX; k_stream_exceed_rows
// widens to int64 on the way to the host.  Levels K..KP-1 hold +inf and stay zero.  Resource usage: profiles/r22_resource_usage.txt.
constexpr int kStreamExceedUnroll = 8;
constexpr int kStreamExceedFields = 5; // count, first, last, longest, current run

template <class T, int KP>
__global__ void __launch_bounds__(kBlock)
k_stream_exceed(const T *__restrict__ q_tm, const int32_t *__restrict__ row_of_pos, const T *__restrict__ th, int32_t *__restrict__ acc,
                int32_t nseg, int64_t nseg_pad, int32_t nsteps, int32_t t0)
{
    static_assert(KP == 1 || KP == 2 || KP == 4, "1, 2 or 4 padded levels");
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    T lim[KP];
    {
        const size_t row = (size_t)row_of_pos[p];
        if constexpr (KP == 1) {
            lim[0] = th[row];
        } else { // (the table's rows are KP * sizeof(T) apart from a 256-byte-aligned base)
            typedef T TV __attribute__((ext_vector_type(KP)));
            const TV x = *reinterpret_cast<const TV *>(th + row * KP);
#pragma unroll
            for (int k = 0; k < KP; ++k) lim[k] = x[k];
        }
    }
    int32_t *const a = acc + p;
    auto at = [&](int f, int k) -> int32_t & { return a[(size_t)(f * KP + k) * (size_t)nseg_pad]; };
    int32_t cnt[KP], first[KP], last[KP], best[KP], run[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        cnt[k] = at(0, k);
        first[k] = at(1, k);
        last[k] = at(2, k);
        best[k] = at(3, k);
        run[k] = at(4, k);
    }
    int32_t tg = t0 + 1; // the step's number in the stream
    auto step = [&](T x) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool over = x > lim[k]; // (ordered compare: false when either side is a NaN)
            cnt[k] += over ? 1 : 0;
            first[k] = (over && first[k] == 0) ? tg : first[k];
            last[k] = over ? tg : last[k];
            run[k] = over ? run[k] + 1 : 0;
            best[k] = max(best[k], run[k]);
        }
        ++tg;
    };
    const T *q = q_tm + (size_t)nseg_pad + p; // (time row 1)
    int32_t t = 1;
    for (; t + kStreamExceedUnroll - 1 <= nsteps; t += kStreamExceedUnroll) {
        T v[kStreamExceedUnroll];
#pragma unroll
        for (int j = 0; j < kStreamExceedUnroll; ++j) v[j] = q[(size_t)(t - 1 + j) * (size_t)nseg_pad];
#pragma unroll
        for (int j = 0; j < kStreamExceedUnroll; ++j) step(v[j]);
    }
    for (; t <= nsteps; ++t) step(q[(size_t)(t - 1) * (size_t)nseg_pad]);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        at(0, k) = cnt[k];
        at(1, k) = first[k];
        at(2, k) = last[k];
        at(3, k) = best[k];
        at(4, k) = run[k];
    }
}

// the accumulator for the host: out[4][nseg][K] int64 in ROW order with exactly the caller's K columns (steps_over, first_step,
// last_step, longest_run), one thread per element
__global__ void __launch_bounds__(kBlock)
k_stream_exceed_rows(const int32_t *__restrict__ acc, const int32_t *__restrict__ pos_of_row, int64_t *__restrict__ out, int32_t nseg,
                     int64_t nseg_pad, int32_t K, int32_t KP)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = (int64_t)nseg * K;
    if (i >= n) return;
    const int32_t r = (int32_t)(i / K), k = (int32_t)(i % K);
    const size_t p = (size_t)pos_of_row[r];
#pragma unroll
    for (int f = 0; f < 4; ++f) out[(size_t)f * (size_t)n + (size_t)i] = acc[(size_t)(f * KP + k) * (size_t)nseg_pad + p];
}
