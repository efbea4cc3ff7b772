// The form rgb32_pack_kernel (handbrake_amd/csrc/rgb_pack.hip) did NOT take, kept for its instruction count only (DESIGN
// 4.6.11): libswscale's own structure - three ramps of packed dwords (the clipped luma ramp shifted to each colour byte's
// place, alpha in the first), here in LDS, and per pixel three reads at Y plus a per-chroma-pair offset and two adds.
// Nothing links this file and nothing runs it:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 --save-temps -c tools/rgb_pack_lds_count.hip -o /dev/null
//     python tools/kernel_isa_count.py rgb_pack_lds_count-hip-amdgcn-amd-amdhsa-gfx950.s rgb32_pack_lds
// The ramps come prebuilt from global memory (RAMP entries a channel, entry k + LOW for ramp index k), which is the cheapest
// way to have them: building them in the kernel costs every lane a few entries' arithmetic for its eight pixels.
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr int RAMP = 768, LOW = 256;           // ramp indices -256 .. 511: Y + the chroma offsets stay inside (|off| <= 236)

struct RgbPackLds
{
    uint8_t       *dst;
    const uint8_t *y, *c0, *c2;
    const uint32_t *ramps;                     // 3 * RAMP packed dwords
    int      dpitch, ypitch, cpitch;
    unsigned lanes, pairs, width;
    int      inc0, inc2, incg0, incg2;         // chroma increments in luma steps, 16.16
    int      bias0, biasg, bias2;              // inc >> 9 of each channel (green: both)
};

__global__ __launch_bounds__(256) void rgb32_pack_lds_kernel(RgbPackLds a)
{
    __shared__ uint32_t ramp[3 * RAMP];
    for (unsigned i = threadIdx.y * 64u + threadIdx.x; i < 3u * RAMP; i += 256u) ramp[i] = a.ramps[i];
    __syncthreads();
    const unsigned lane = blockIdx.x * 64u + threadIdx.x, pair = blockIdx.y * 4u + threadIdx.y;
    if (lane >= a.lanes || pair >= a.pairs) return;
    const uint8_t *yrow = a.y + (size_t)(2 * pair) * a.ypitch + (size_t)lane * 4;
    const unsigned y0 = *reinterpret_cast<const unsigned *>(yrow);
    const unsigned y1 = *reinterpret_cast<const unsigned *>(yrow + a.ypitch);
    const size_t cat = (size_t)pair * a.cpitch + (size_t)lane * 2;
    const unsigned p0 = *reinterpret_cast<const uint16_t *>(a.c0 + cat);
    const unsigned p2 = *reinterpret_cast<const uint16_t *>(a.c2 + cat);
    unsigned top[4], bot[4];
#pragma unroll
    for (int k = 0; k < 2; k++)
    {
        const int s0 = (int)((p0 >> (8 * k)) & 255u), s2 = (int)((p2 >> (8 * k)) & 255u);
        const uint32_t *r0 = ramp + LOW + (__mul24(s0, a.inc0) >> 16) - a.bias0;
        const uint32_t *r2 = ramp + 2 * RAMP + LOW + (__mul24(s2, a.inc2) >> 16) - a.bias2;
        const uint32_t *rg = ramp + RAMP + LOW + (__mul24(s0, a.incg0) >> 16) + (__mul24(s2, a.incg2) >> 16) - a.biasg;
#pragma unroll
        for (int j = 2 * k; j < 2 * k + 2; j++)
        {
            const unsigned ya = (y0 >> (8 * j)) & 255u, yb = (y1 >> (8 * j)) & 255u;
            top[j] = r0[ya] + rg[ya] + r2[ya];
            bot[j] = r0[yb] + rg[yb] + r2[yb];
        }
    }
    uint8_t *d = a.dst + (size_t)(2 * pair) * a.dpitch + (size_t)lane * 16;
    if (lane * 4u + 4u <= a.width)
    {
        *reinterpret_cast<uint4 *>(d) = make_uint4(top[0], top[1], top[2], top[3]);
        *reinterpret_cast<uint4 *>(d + a.dpitch) = make_uint4(bot[0], bot[1], bot[2], bot[3]);
    }
    else
    {
        *reinterpret_cast<uint2 *>(d) = make_uint2(top[0], top[1]);
        *reinterpret_cast<uint2 *>(d + a.dpitch) = make_uint2(bot[0], bot[1]);
    }
}

} // namespace

// keeps the kernel in the object
void *rgb32_pack_lds_kernel_address() { return (void *)rgb32_pack_lds_kernel; }
