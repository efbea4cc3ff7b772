// eedi2_mask_cells.h - the part of the fused EEDI2 mask kernels that never sees a sample: erode / dilate / erode and
// remove_small_gaps on the LDS frame of mask cells (eedi2_template.c:207-342).  Shared by mask_tile (eedi2.hip, 8-bit
// samples) and qmask_tile (eedi2_16.hip, 10 / 12-bit samples), which keep their own staging, edge tests and stores.
//
// Every value of the mask is 0 or peak at any depth, so inside the kernels a mask cell is one byte holding 0 / 1 and
// four of them are handled by one 32-bit operation: the 8-neighbour count of erode / dilate is a sum of byte-shifted
// dwords (at most 8 per byte, no carries), the threshold test one add (bit 7 of count + 0x80 - thr), remove_small_gaps
// a handful of ANDs / ORs of shifted dwords.  A thread owns one dword column of the LDS frame and a strip of SR rows; it
// loads the SR + 2 rows x 3 dwords around the strip once and keeps the per-row partial sums in registers.  Each pass
// computes the whole frame minus one more row top and bottom; the cells next to the frame's left / right edge come out
// wrong by design (they read the unwritten pad column), one byte further in per pass, which the 8-byte column halo
// absorbs (the tile needs x0 - 3 .. x0 + W + 2 from the last erode).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// A mask tile of TILE_W x TILE_H cells on THREADS threads, STRIP_ROWS rows per thread and pass, and its LDS frame
template <int TILE_W, int TILE_H, int STRIP_ROWS, int THREADS>
struct EediMaskGeo
{
    static constexpr int W = TILE_W, H = TILE_H, OX = 8, OY = 4;      // tile and the LDS frame's origin offset
    static constexpr int LP = W + 2 * OX, LR = H + 2 * OY;            // the LDS frame (64 x 16: 80 x 24, 128 x 16: 144 x 24)
    static constexpr int DW = LP / 4;                                 // dwords per LDS row
    static constexpr int DP = DW + 2;                                 // + one pad dword either side
    static constexpr int SR = STRIP_ROWS;                             // rows per thread and pass
    static constexpr int T = THREADS;
    static_assert(((LR - 2 + SR - 1) / SR) * DW <= T, "a thread per strip and dword column");
};

// (internal to the file that includes this header, like the kernels that use them)
namespace {

// 0xff in byte k when lo <= X + k < hi
__device__ __forceinline__ uint32_t bytes_in(int X, int lo, int hi)
{
    uint32_t m = 0xffffffffu;
    const int a = lo - X, b = hi - X;
    if (a > 0) m = a >= 4 ? 0u : (m << (8 * a));
    if (b < 4) m = b <= 0 ? 0u : (m & (0xffffffffu >> (8 * (4 - b))));
    return m;
}

// erode (GROW = false) / dilate (GROW = true) of LDS rows ra .. rb
template <typename Geo, bool GROW>
__device__ __forceinline__ void morph4(const uint32_t (*src)[Geo::DP], uint32_t (*dst)[Geo::DP], int c4, int strip,
                                       int ra, int rb, int thr, uint32_t px1, int fy, int height)
{
    constexpr int SR = Geo::SR;
    const int r0 = ra + strip * SR;
    if (r0 <= rb)
    {
        const uint32_t K = (uint32_t)(0x80 - min(max(thr, 0), 9)) * 0x01010101u;
        uint32_t S2[SR + 2], S3[SR + 2], C[SR + 2];
#pragma unroll
        for (int i = 0; i < SR + 2; i++)
        {
            const int r = min(r0 - 1 + i, Geo::LR - 1);
            const uint32_t l = src[r][c4], c = src[r][c4 + 1], rr = src[r][c4 + 2];
            const uint32_t lb = __builtin_amdgcn_alignbyte(c, l, 3), rbv = __builtin_amdgcn_alignbyte(rr, c, 1);
            C[i] = c;
            S2[i] = lb + rbv;
            S3[i] = S2[i] + c;
        }
#pragma unroll
        for (int i = 0; i < SR; i++)
        {
            const int r = r0 + i;
            if (r > rb) break;
            const int y = fy + r;
            const uint32_t count = S3[i] + S2[i + 1] + S3[i + 2];
            const uint32_t ge = ((count + K) >> 7) & 0x01010101u;          // count >= thr, per cell
            const uint32_t pm = (y >= 1 && y < height - 1) ? px1 : 0u;
            const uint32_t c = C[i + 1];
            dst[r][c4 + 1] = GROW ? (c | (ge & pm)) : (c & ~((ge ^ 0x01010101u) & pm));
        }
    }
    __syncthreads();
}

// remove_small_gaps (:308-342) on four cells: l, c, rr the dwords left of, at and right of them, pm the cells the pass
// processes (0x01 each; the others keep their input).  Returns 0 / 1 per cell.
__device__ __forceinline__ uint32_t small_gaps4(uint32_t l, uint32_t c, uint32_t rr, uint32_t pm)
{
    const uint32_t a1 = __builtin_amdgcn_alignbyte(c, l, 3), a2 = __builtin_amdgcn_alignbyte(c, l, 2), a3 = __builtin_amdgcn_alignbyte(c, l, 1);
    const uint32_t b1 = __builtin_amdgcn_alignbyte(rr, c, 1), b2 = __builtin_amdgcn_alignbyte(rr, c, 2), b3 = __builtin_amdgcn_alignbyte(rr, c, 3);
    const uint32_t a12 = a1 | a2, a123 = a12 | a3;
    const uint32_t set = c & (a123 | b1 | b2 | b3);                               // a set cell survives with any neighbour set
    const uint32_t fill = ((b1 & a123) | (b2 & a12) | (b3 & a1)) & (c ^ 0x01010101u);
    return ((set | fill) & pm) | (c & ~pm);
}

} // namespace
