// k_stream_exceed_depth -- OUT-OF-BANK AND STAGE-THRESHOLD EXCEEDANCE OVER A WHOLE STREAM OF DAYS (trmc_stream_set_depth_exceedance,
// trmc_stream_depth_exceedance; launched by stream_complete_day, stream.inc, beside k_stream_exceed and k_stream_courant).  The
// definition is k_stream_exceed's (k_stream_exceed.inc, k_window_exceed.inc), on DEPTH: over(t) := d[t] > th[row][k], compared in T
// -- false when either side is a NaN, equality is not over -- and per row and level steps_over, first_step, last_step, longest_run
// with t counted on over the days, 1-based from the stream's first step; a run that is open at a day's last step goes on at the
// next day's first, so the state lives in an accumulator of its own outside the ring and this kernel folds one day into it, in day
// order.  d[t] is the depth the stream holds for the row and step -- what stage and the full result hand out: the pool's water
// elevation at a reservoir row, 0 at a boundary row (nobody routes it: the planes and the result are zeroed, stream_begin_t), the
// step's own depth at a gage row.
//
// A SECOND ACCUMULATOR, NOT A QUANTITY OF THE FIRST: its thresholds are metres and belong to the stream (StreamRun::dex_th), the flow
// fold's are m3/s and belong to the plan, and one stream may keep both.  The flow kernel is left as it is -- its body is written
// again here rather than shared, so that its generated code stays what profiles/r22_resource_usage.txt records.
//
// WALK: k_stream_exceed's.  One thread per plan position, time runs in the thread, kStreamExceedUnroll independent loads are issued
// before the first compare that depends on them.  DEPTH OF STEP t of position p: d1[x * d_row + (t - 1) * d_step] with
// (x, d_row, d_step) = (p, 1, nseg_pad) on the slot's depth plane from time row 1 -- a wavefront's load is 64 consecutive depths of
// a time row -- or (row_of_pos[p], 3 nsteps, 3) on the day's full result out[row][step][2] (by_row): k_stream_courant's pair.  The
// second is strided by 3 nsteps elements per lane: every lane walks a row of its own, a wavefront's load touches 64 lines, and a
// third of every line fetched is depth -- three times the plane's bytes at best, uncoalesced; the path of a stream that already
// pays for the full result (measured: profiles/r28_stream_depth_exceedance_ab.txt).
// THRESHOLDS: [nseg][KP] in ROW order, KP in {1, 2, 4}, +inf -- never over -- behind the K levels asked for, ONE vector load per row
// through row_of_pos from a 256-byte-aligned base.
// STATE: int32 acc[5][KP][nseg_pad] in PLAN order -- count, first, last, longest, current run -- read once and written once per row
// and day; trmc_stream_push_day refuses the day that would take the stream's step count past INT32_MAX;
// k_stream_exceed_depth_rows brings it into row order and widens to int64 on the way to the host.  Levels K..KP-1 hold +inf and stay
// zero.  Resource usage: profiles/r28_resource_usage.txt.
template <class T, int KP>
__global__ void __launch_bounds__(kBlock)
k_stream_exceed_depth(const T *__restrict__ d1, const int32_t *__restrict__ row_of_pos, const T *__restrict__ th, int32_t *__restrict__ acc,
                      int32_t nseg, int64_t nseg_pad, int32_t nsteps, int32_t t0, int32_t by_row, int64_t d_row, int64_t d_step)
{
    static_assert(KP == 1 || KP == 2 || KP == 4, "1, 2 or 4 padded levels");
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const size_t row = (size_t)row_of_pos[p];
    T lim[KP];
    if constexpr (KP == 1) {
        lim[0] = th[row];
    } else { // (the table's rows are KP * sizeof(T) apart from a 256-byte-aligned base)
        typedef T TV __attribute__((ext_vector_type(KP)));
        const TV x = *reinterpret_cast<const TV *>(th + row * KP);
#pragma unroll
        for (int k = 0; k < KP; ++k) lim[k] = x[k];
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
    const T *const d = d1 + (by_row ? row : (size_t)p) * (size_t)d_row; // (step 1)
    const size_t ds = (size_t)d_step;
    int32_t t = 1;
    for (; t + kStreamExceedUnroll - 1 <= nsteps; t += kStreamExceedUnroll) {
        T v[kStreamExceedUnroll];
#pragma unroll
        for (int j = 0; j < kStreamExceedUnroll; ++j) v[j] = d[(size_t)(t - 1 + j) * ds];
#pragma unroll
        for (int j = 0; j < kStreamExceedUnroll; ++j) step(v[j]);
    }
    for (; t <= nsteps; ++t) step(d[(size_t)(t - 1) * ds]);
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
k_stream_exceed_depth_rows(const int32_t *__restrict__ acc, const int32_t *__restrict__ pos_of_row, int64_t *__restrict__ out, int32_t nseg,
                           int64_t nseg_pad, int32_t K, int32_t KP)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = (int64_t)nseg * K;
    if (i >= n) return;
    const int32_t r = (int32_t)(i / K), k = (int32_t)(i % K);
    const size_t p = (size_t)pos_of_row[r];
#pragma unroll
    for (int f = 0; f < 4; ++f) out[(size_t)f * (size_t)n + (size_t)i] = acc[(size_t)(f * KP + k) * (size_t)nseg_pad + p];
}
