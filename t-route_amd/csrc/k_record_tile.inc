// k_record_tile -- the walk over a window's assembled result out[nseg][nsteps][3] = (q, v, d) per step, row-major, that the per-row
// products of a finished window share (k_window_summary, k_window_exceed): a tile of rows goes through LDS chunk by chunk, and
// each lane hands ITS row's steps, in step order, to the kernel's own step function.
//
// TILING.  A row's record is nsteps * 3 contiguous elements (3 456 B at 288 fp32 steps): a thread per row striding through it makes
// every wavefront load touch 64 cache lines.  Here a block of ONE wavefront owns kRecRows = 64 rows and walks their records in
// chunks of kRecSteps<T> = 128 / sizeof(T) steps (32 fp32, 16 fp64): a row's chunk is 384 contiguous bytes -- three 128-byte
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
//   walk   lane r walks row r's chunk in step order, three vectors (VE = 16 / sizeof(T) steps) at a time, the kernel's running
//          values in registers from chunk to chunk.  The next chunk's 24 loads are issued BEFORE the walk and land during it; one
//          wavefront per block makes the two barriers per chunk cheap.  The summary's ~330 VALU instructions per 24 KiB are an
//          order of magnitude under what the memory system asks for (13 B per clock per compute unit at 8 TB/s).
// One wavefront with 24 vectors (96 VGPRs) in flight, 6 blocks per compute unit: 144 KiB outstanding per compute unit, above the
// ~64 KiB that 8 TB/s times a 2 us latency needs.  Resource usage of the kernels built on it: profiles/r23_resource_usage.txt (160
// VGPRs the summary, no scratch).  Measured at CONUS size (2 729 077 rows x 288 fp32 steps, 9.43 GB), the summary: 1.55 ms = 6.1 TB/s,
// 1.32 x the bytes at 8 TB/s (profiles/r18_window_summary_ab.txt); both kernels before and after they shared this file:
// profiles/r23_window_tile_ab.txt.
constexpr int kRecRows = 64;
template <class T> constexpr int kRecSteps = 128 / (int)sizeof(T);
constexpr int kRecChunkBytes = 384, kRecPitchBytes = kRecChunkBytes + 16;
template <class T> using RecVec = T __attribute__((ext_vector_type(16 / sizeof(T)))); // 16 bytes: float4 / double2
constexpr int kRecTileVecs = kRecRows * (kRecPitchBytes / 16);                         // the tile in LDS, in vectors

// The kernel -- a block of kRecRows threads -- declares  __shared__ RecVec<T> s_tile[kRecTileVecs];  __shared__ int64_t
// s_src[kRecRows];  puts into s_src[lane] the element offset of its row's record in `out` (-1 beyond the last row: `mine` false)
// and passes a __syncthreads().  Then, for a lane that is `mine`:  first(q, v, d) once with step 1's triple, before any step;
// step(q, v, d) for every step 1..nsteps, in step order.  Every lane of the block must call it (it holds barriers).
template <class T, bool VEC, class First, class Step>
__device__ __forceinline__ void record_tile_walk(const T *__restrict__ out, RecVec<T> *s_tile, const int64_t *s_src, bool mine,
                                                 int32_t nsteps, First &&first, Step &&step)
{
    typedef RecVec<T> V;
    constexpr int VE = 16 / (int)sizeof(T);           // elements of a vector = steps of a group of three vectors
    constexpr int C = kRecSteps<T>;                   // steps of a chunk
    constexpr int CV = kRecChunkBytes / 16;           // vectors of a row's chunk (24)
    constexpr int PV = kRecPitchBytes / 16;           // LDS row pitch in vectors (25)
    constexpr int PE = kRecPitchBytes / (int)sizeof(T), CE = 3 * C; // ... and in elements; elements of a row's chunk
    constexpr int NV = CV;                            // vectors a lane stages per chunk: 64 rows x 24 / 64 lanes
    const int lane = threadIdx.x;
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
            for (int j = lane; j < kRecRows * CE; j += kRecRows) {
                const int r = j / CE, c = j - r * CE;
                const int64_t src = s_src[r];
                if (src >= 0 && c < ne) s_elem[r * PE + c] = out[src + (int64_t)c0 * 3 + c];
            }
        }
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
            if (c0 == 0) first(re[0], re[1], re[2]);
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
}
