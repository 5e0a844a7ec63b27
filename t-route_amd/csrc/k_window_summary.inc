// k_window_summary -- one pass over a window's assembled result out[nseg][nsteps][3] = (q, v, d) per step, row-major, that leaves
// per row: peak flow / depth / velocity with the 1-based step each was FIRST reached at, and the mean flow (trmc_window_summary,
// abi.inc).  Same compares and the same left-to-right sum in T as k_stream_summary / k_stream_peak_depth_out, so a window and a
// one-day stream give the same bits:  pk = x[1], at = 1;  t = 2..nsteps: if (x[t] > pk) { pk = x[t]; at = t; }   (the first of
// equal peaks wins, a NaN never replaces a number);  mean = (((x[1] + x[2]) + ...) + x[nsteps]) / T(nsteps).
//
// TILING.  A row's record is nsteps * 3 contiguous elements (3 456 B at 288 fp32 steps): a thread per row striding through it makes
// every wavefront load touch 64 cache lines.  Here a block of ONE wavefront owns kWsumRows = 64 rows and walks their records in
// chunks of kWsumSteps<T> = 128 / sizeof(T) steps (32 fp32, 16 fp64): a row's chunk is 384 contiguous bytes -- three 128-byte
// lines, line-aligned wherever the record is (288 fp32 steps: 27 lines a row) -- whatever the precision.
//   load   the tile's 64 x 384 B go global -> registers as 24 16-byte vectors per lane and from there to LDS with 16-byte stores.
//          Eight consecutive lanes take one 128-byte line of a row's chunk; a wave-load is one whole line of each of 8 rows (rows
//          lane / 8 + 8 b, b = 0..7), and the chunk's three lines are the same address plus 0 / 128 / 256 B: eight row pointers a
//          lane, everything else immediates.  16-byte loads need every row's record 16-byte aligned: nsteps % 4 == 0 (fp32) /
//          nsteps % 2 == 0 (fp64), and then every chunk -- the last, short one too -- is a whole number of vectors.  Any other
//          nsteps: the same tile element by element (VEC = false), consecutive lanes on consecutive elements.
//   LDS    row pitch 400 B = 384 + one 16-byte slot of padding.  The walk reads 16 bytes per lane (ds_read_b128: banks (a / 4) mod
//          64, four groups of 16 lanes): lane r sits at dword 100 r + k, slot (9 r) mod 16 of the 256-byte bank row -- 16 lanes whose
//          r mod 16 are all different (every one of the instruction's lane groups) hit 16 different slots: conflict-free.  The
//          staging stores put 8 consecutive lanes (the 16-byte store's lane group) on the 32 consecutive dwords of a line.  Tile: 64 x 400 B = 25 KiB, six blocks on a compute unit's 160 KiB.
//   walk   lane r walks row r's chunk in step order, three vectors (VE = 16 / sizeof(T) steps) at a time, the seven running values
//          in registers from chunk to chunk.  The next chunk's 24 loads are issued BEFORE the walk and land during it; one
//          wavefront per block makes the two barriers per chunk cheap.  ~330 VALU instructions per 24 KiB: an order of magnitude
//          under what the memory system asks for (13 B per clock per compute unit at 8 TB/s).
// One wavefront with 24 vectors (96 VGPRs) in flight, 6 blocks per compute unit: 144 KiB outstanding per compute unit, above the
// ~64 KiB that 8 TB/s times a 2 us latency needs.  Resource usage: profiles/r18_resource_usage.txt (160 VGPRs, no scratch).  Measured at
// CONUS size (2 729 077 rows x 288 fp32 steps, 9.43 GB): 1.55 ms = 6.1 TB/s, 1.32 x the bytes at 8 TB/s (profiles/r18_window_summary_ab.txt).
//
// `rowset_pos` (NULL: output i = row i): plan positions of a registered set (trmc_rowset_create), row_of_pos takes them to rows of
// `out`; output i is the set's i-th row.  Any of the seven outputs may be NULL.
constexpr int kWsumRows = 64;
template <class T> constexpr int kWsumSteps = 128 / (int)sizeof(T);
constexpr int kWsumChunkBytes = 384, kWsumPitchBytes = kWsumChunkBytes + 16;

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
__global__ void __launch_bounds__(kWsumRows, 2)
k_window_summary(const T *__restrict__ out, const int32_t *__restrict__ rowset_pos, const int32_t *__restrict__ row_of_pos, WsumOut<T> o,
                 int64_t nrows, int32_t nsteps)
{
    typedef T V __attribute__((ext_vector_type(16 / sizeof(T)))); // 16 bytes: float4 / double2
    constexpr int VE = 16 / (int)sizeof(T);           // elements of a vector = steps of a group of three vectors
    constexpr int C = kWsumSteps<T>;                  // steps of a chunk
    constexpr int CV = kWsumChunkBytes / 16;          // vectors of a row's chunk (24)
    constexpr int PV = kWsumPitchBytes / 16;          // LDS row pitch in vectors (25)
    constexpr int PE = kWsumPitchBytes / (int)sizeof(T), CE = 3 * C; // ... and in elements; elements of a row's chunk
    constexpr int NV = CV;                            // vectors a lane stages per chunk: 64 rows x 24 / 64 lanes
    __shared__ V s_tile[kWsumRows * PV];
    __shared__ int64_t s_src[kWsumRows];              // element offset of the tile's rows in `out`, -1 beyond the last row
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kWsumRows + lane;
    const bool mine = i < nrows;
    {
        int64_t row = -1;
        if (mine) row = rowset_pos ? (int64_t)row_of_pos[rowset_pos[i]] : i;
        s_src[lane] = row < 0 ? -1 : row * (int64_t)nsteps * 3;
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
            for (int j = lane; j < kWsumRows * CE; j += kWsumRows) {
                const int r = j / CE, c = j - r * CE;
                const int64_t src = s_src[r];
                if (src >= 0 && c < ne) s_elem[r * PE + c] = out[src + (int64_t)c0 * 3 + c];
            }
        }
    };

    T pq = T(0), pv = T(0), pd = T(0);
    T sum = T(-0.0); // (-0 + x == x for every x, a -0 included: the sum starts AT x[1], as np.cumsum does)
    int32_t aq = 1, av = 1, ad = 1, t = 1;
    auto step = [&](T q, T v, T d) {
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
            if (c0 == 0) { // the peaks start at step 1 (the compares of step 1 against itself below change nothing)
                pq = re[0];
                pv = re[1];
                pd = re[2];
            }
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
                for (int m = 0; m < VE; ++m) step(e[3 * m], e[3 * m + 1], e[3 * m + 2]);
            }
            for (; g < cl; ++g) step(re[3 * g], re[3 * g + 1], re[3 * g + 2]);
        }
        __syncthreads();
    }
    if (!mine) return;
    if (o.peak_flow) o.peak_flow[i] = pq;
    if (o.peak_step) o.peak_step[i] = aq;
    if (o.mean_flow) o.mean_flow[i] = sum / T(nsteps);
    if (o.peak_depth) o.peak_depth[i] = pd;
    if (o.peak_depth_step) o.peak_depth_step[i] = ad;
    if (o.peak_velocity) o.peak_velocity[i] = pv;
    if (o.peak_velocity_step) o.peak_velocity_step[i] = av;
}
