// jpeg_block.h — one 8 x 8 block of the preview JPEG (jpeg.hip): libjpeg's accurate integer forward DCT
// (jfdctint.c: 13-bit constants, PASS1_BITS 2, rows first), its quantisation, and the block's Huffman symbols.  The same
// text runs in the kernels and on the host (tools/jpeg_block_check, tests/test_preview_jpeg_cpu.py), like lapsharp_rowdot.h.
//
// Everything is written for full unrolling: a block lives in 64 registers and every index is a constant after it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#define JPB_FN __host__ __device__ __forceinline__

#define JPB_MAX_BLOCK_BITS 1660             // DC 11 + 11, 63 x (AC 16 + 10)
#define JPB_SLOT_BYTES     256              // a block's bit string in device memory (jpeg.hip)

// natural index of the k-th coefficient of the scan
#define JPB_ZIGZAG { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
                     28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, \
                     54, 47, 55, 62, 63 }

// ---- tables: Annex K of T.81, built on the host ----
struct JpbHuffSpec { uint8_t bits[16]; uint8_t vals[162]; int nvals; };

// code | length << 16 per symbol (0: no such symbol); [0] luma, [1] chroma
struct JpbTables
{
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint16_t divisor[2][64];                // q << 3, natural order
};

static inline const JpbHuffSpec *jpb_huff_spec(int cls, int id)
{
    static const JpbHuffSpec dc_luma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
    static const JpbHuffSpec dc_chroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
    static const JpbHuffSpec ac_luma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
        0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
        0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
        0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
        0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
        0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa}, 162};
    static const JpbHuffSpec ac_chroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
        0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
        0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
        0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
        0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa}, 162};
    return cls == 0 ? (id == 0 ? &dc_luma : &dc_chroma) : (id == 0 ? &ac_luma : &ac_chroma);
}

// Annex K.1's bases scaled by jpeg_quality_scaling / jpeg_add_quant_table (baseline); natural order
static inline void jpb_quant_table(int chroma, int quality, uint8_t q[64])
{
    static const uint8_t base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; i++)
    {
        const int v = (base[chroma][i] * s + 50) / 100;
        q[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

static inline void jpb_code_table(const JpbHuffSpec *spec, uint32_t *table, int entries)
{
    for (int i = 0; i < entries; i++) table[i] = 0;
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++)
    {
        for (int i = 0; i < spec->bits[len - 1]; i++, k++, code++)
            if (spec->vals[k] < entries) table[spec->vals[k]] = code | ((uint32_t)len << 16);
        code <<= 1;
    }
}

static inline void jpb_tables(int quality, JpbTables *t)
{
    for (int c = 0; c < 2; c++)
    {
        jpb_code_table(jpb_huff_spec(0, c), t->dc[c], 16);
        jpb_code_table(jpb_huff_spec(1, c), t->ac[c], 256);
        uint8_t q[64];
        jpb_quant_table(c, quality, q);
        for (int i = 0; i < 64; i++) t->divisor[c][i] = (uint16_t)(q[i] << 3);
    }
}

// ---- the transform ----
JPB_FN int jpb_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass over d[0], d[S], .. d[7 S]; FIRST: rows (results scaled up by 4), else columns (the final descale)
template <bool FIRST, int S>
JPB_FN void jpb_fdct_pass(int *d)
{
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S];
    const int t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S];
    const int t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    d[0] = FIRST ? (t10 + t11) * 4 : jpb_descale(t10 + t11, 2);
    d[4 * S] = FIRST ? (t10 - t11) * 4 : jpb_descale(t10 - t11, 2);
    const int e1 = (t12 + t13) * 4433;
    d[2 * S] = jpb_descale(e1 + t13 * 6270, N);
    d[6 * S] = jpb_descale(e1 + t12 * -15137, N);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995;
    const int z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d[7 * S] = jpb_descale(t4 * 2446 + z1 + z3, N);
    d[5 * S] = jpb_descale(t5 * 16819 + z2 + z4, N);
    d[3 * S] = jpb_descale(t6 * 25172 + z2 + z3, N);
    d[S] = jpb_descale(t7 * 12299 + z1 + z4, N);
}

// d: the block's samples less 128, natural order; out: 8 x the DCT
JPB_FN void jpb_fdct_islow(int d[64])
{
#pragma unroll
    for (int r = 0; r < 8; r++) jpb_fdct_pass<true, 1>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; c++) jpb_fdct_pass<false, 8>(d + c);
}

// |c| + (d >> 1) over d = q << 3, truncating, the sign put back
JPB_FN int jpb_quantize(int c, int divisor)
{
    const unsigned mag = ((unsigned)(c < 0 ? -c : c) + ((unsigned)divisor >> 1)) / (unsigned)divisor;
    return c < 0 ? -(int)mag : (int)mag;
}

// ---- the entropy code ----
// (category, the value's low bits: v, or v - 1 for a negative one)
JPB_FN int jpb_category(int v)
{
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    n = 32 - __clz((int)a);
#else
    while (a) { n++; a >>= 1; }
#endif
    return n;
}

// A block's symbols into `sink` (sink.put(bits, length), length 1 .. 16, the code and the value bits apart); coef(k): the
// k-th coefficient of the scan, k a constant after unrolling.  Returns nothing: the block's DC is coef(0).
template <class Coef, class Sink>
JPB_FN void jpb_code_block(Coef coef, int pred, const uint32_t *dc_table, const uint32_t *ac_table, Sink &sink)
{
    {
        const int diff = coef(0) - pred;
        const int n = jpb_category(diff);
        const uint32_t e = dc_table[n];
        sink.put(e & 0xffffu, (int)(e >> 16));
        if (n) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; k++)
    {
        const int v = coef(k);
        if (v == 0) { run++; continue; }
        while (run > 15)
        {
            const uint32_t z = ac_table[0xf0];
            sink.put(z & 0xffffu, (int)(z >> 16));
            run -= 16;
        }
        const int n = jpb_category(v);
        const uint32_t e = ac_table[((run << 4) | n) & 0xff];
        sink.put(e & 0xffffu, (int)(e >> 16));
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
        run = 0;
    }
    if (run)
    {
        const uint32_t e = ac_table[0];
        sink.put(e & 0xffffu, (int)(e >> 16));
    }
}

// a block of an MCU that lies outside its component's real blocks: DC difference 0, end of block
template <class Sink>
JPB_FN void jpb_code_dummy(const uint32_t *dc_table, const uint32_t *ac_table, Sink &sink)
{
    sink.put(dc_table[0] & 0xffffu, (int)(dc_table[0] >> 16));
    sink.put(ac_table[0] & 0xffffu, (int)(ac_table[0] >> 16));
}

// ---- where a block of the scan lies ----
// MCUs of 16 x 16 luma samples in raster order, each Y00 Y01 Y10 Y11 Cb Cr: block b is block b % 6 of MCU b / 6.
struct JpbGeom
{
    int width, height;                      // luma, both even
    int mcus_w, mcus_h;                     // ceil(width / 16), ceil(height / 16)
    int real_w, real_h;                     // luma blocks that hold samples: ceil(width / 8), ceil(height / 8)
};

static inline JpbGeom jpb_geom(int width, int height)
{
    JpbGeom g;
    g.width = width; g.height = height;
    g.mcus_w = (width + 15) / 16; g.mcus_h = (height + 15) / 16;
    g.real_w = (width + 7) / 8; g.real_h = (height + 7) / 8;
    return g;
}

struct JpbPlace { int comp, bx, by; bool dummy; };

JPB_FN JpbPlace jpb_place(const JpbGeom &g, int b)
{
    const int m = b / 6, k = b - 6 * m;
    const int my = m / g.mcus_w, mx = m - my * g.mcus_w;
    JpbPlace p;
    if (k < 4)
    {
        p.comp = 0; p.bx = 2 * mx + (k & 1); p.by = 2 * my + (k >> 1);
        p.dummy = p.bx >= g.real_w || p.by >= g.real_h;       // only luma has such blocks at 4:2:0
    }
    else
    {
        p.comp = k - 3; p.bx = mx; p.by = my; p.dummy = false;
    }
    return p;
}

// the block whose DC predicts block b's: the component's previous block of the scan that is not a dummy (an MCU's Y00 never
// is one, so the walk is three steps at the most); -1: the component's first block, predicted from 0
JPB_FN int jpb_pred_block(const JpbGeom &g, int b)
{
    const int m = b / 6, k = b - 6 * m;
    if (k >= 4) return m > 0 ? b - 6 : -1;
    int p = k > 0 ? b - 1 : b - 3;                            // Y11 of the MCU before
    while (p >= 0 && jpb_place(g, p).dummy) p--;
    return p;
}

// The samples of block (bx, by) of a pw x ph plane less 128, the plane continued by its last column and row.  The block
// holds samples (8 bx < pw, 8 by < ph); rows are read as two dwords: the plane starts on and its pitch is a multiple of 8
// bytes, at least pw rounded up to 8.
JPB_FN void jpb_load_block(const uint8_t *plane, int pitch, int pw, int ph, int bx, int by, int d[64])
{
    const int last = pw - 1 - 8 * bx;                         // the block's column of the plane's last sample (>= 0)
#pragma unroll
    for (int r = 0; r < 8; r++)
    {
        const int y = 8 * by + r < ph ? 8 * by + r : ph - 1;
        const uint32_t *row = reinterpret_cast<const uint32_t *>(plane + (size_t)y * pitch + 8 * bx);
        const uint32_t lo = row[0], hi = row[1];
        int s[8];
#pragma unroll
        for (int c = 0; c < 8; c++) s[c] = (int)(((c < 4 ? lo : hi) >> (8 * (c & 3))) & 0xffu);
        if (last < 7)
        {
            int edge = s[0];
#pragma unroll
            for (int c = 1; c < 8; c++) edge = c == last ? s[c] : edge;
#pragma unroll
            for (int c = 1; c < 8; c++) s[c] = c > last ? edge : s[c];
        }
#pragma unroll
        for (int c = 0; c < 8; c++) d[8 * r + c] = s[c] - 128;
    }
}

// a real block from samples to its quantised coefficients in scan order: zz[k], k = 0 .. 63
JPB_FN void jpb_transform_block(int d[64], const uint16_t *divisor, int16_t zz[64])
{
    constexpr int order[64] = JPB_ZIGZAG;
    jpb_fdct_islow(d);
#pragma unroll
    for (int k = 0; k < 64; k++) zz[k] = (int16_t)jpb_quantize(d[order[k]], divisor[order[k]]);
}
