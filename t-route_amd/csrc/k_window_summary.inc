// k_window_summary -- one pass over a window's assembled result out[nseg][nsteps][3] = (q, v, d) per step, row-major, that leaves
// per row: peak flow / depth / velocity with the 1-based step each was FIRST reached at, and the mean flow (trmc_window_summary,
// abi.inc).  Same compares and the same left-to-right sum in T as k_stream_summary / k_stream_peak_depth_out, so a window and a
// one-day stream give the same bits:  pk = x[1], at = 1;  t = 2..nsteps: if (x[t] > pk) { pk = x[t]; at = t; }   (the first of
// equal peaks wins, a NaN never replaces a number);  mean = (((x[1] + x[2]) + ...) + x[nsteps]) / T(nsteps).
//
// TILING: k_record_tile.inc's record_tile_walk (whose head has the reasons, the LDS bank arithmetic and the measured figures).  Here
// the seven running values of a lane's row and what each step does to them.
//
// `rowset_pos` (NULL: output i = row i): plan positions of a registered set (trmc_rowset_create), row_of_pos takes them to rows of
// `out`; output i is the set's i-th row.  Any of the seven outputs may be NULL.
template <class T> struct WsumOut {
    T *peak_flow;
    int32_t *peak_step;
    T *mean_flow;
    T *peak_depth;
    int32_t *peak_depth_step;
    T *peak_velocity;
    int32_t *peak_velocity_step;
};

template <class T, bool VEC>
__global__ void __launch_bounds__(kRecRows, 2)
k_window_summary(const T *__restrict__ out, const int32_t *__restrict__ rowset_pos, const int32_t *__restrict__ row_of_pos, WsumOut<T> o,
                 int64_t nrows, int32_t nsteps)
{
    __shared__ RecVec<T> s_tile[kRecTileVecs];
    __shared__ int64_t s_src[kRecRows];               // element offset of the tile's rows in `out`, -1 beyond the last row
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kRecRows + lane;
    const bool mine = i < nrows;
    {
        int64_t row = -1;
        if (mine) row = rowset_pos ? (int64_t)row_of_pos[rowset_pos[i]] : i;
        s_src[lane] = row < 0 ? -1 : row * (int64_t)nsteps * 3;
    }
    __syncthreads();

    T pq = T(0), pv = T(0), pd = T(0);
    T sum = T(-0.0); // (-0 + x == x for every x, a -0 included: the sum starts AT x[1], as np.cumsum does)
    int32_t aq = 1, av = 1, ad = 1, t = 1;
    record_tile_walk<T, VEC>(
        out, s_tile, s_src, mine, nsteps,
        [&](T q, T v, T d) { // the peaks start at step 1 (the compares of step 1 against itself below change nothing)
            pq = q;
            pv = v;
            pd = d;
        },
        [&](T q, T v, T d) {
            if (q > pq) {
                pq = q;
                aq = t;
            }
            if (v > pv) {
                pv = v;
                av = t;
            }
            if (d > pd) {
                pd = d;
                ad = t;
            }
            sum += q;
            ++t;
        });
    if (!mine) return;
    if (o.peak_flow) o.peak_flow[i] = pq;
    if (o.peak_step) o.peak_step[i] = aq;
    if (o.mean_flow) o.mean_flow[i] = sum / T(nsteps);
    if (o.peak_depth) o.peak_depth[i] = pd;
    if (o.peak_depth_step) o.peak_depth_step[i] = ad;
    if (o.peak_velocity) o.peak_velocity[i] = pv;
    if (o.peak_velocity_step) o.peak_velocity_step[i] = av;
}
