// jpeg.hip — the JPEG the title scan stores for a preview (libhb/scan.c:979-982 -> hb_save_preview, hb.c:583-629), written on
// gfx950 for pictures that are in HBM already: the picture stays where it is and the finished scan segment comes back
// instead of the planes.  8-bit planar 4:2:0 with even sizes, which is what the scan decodes to (decavcodec.c:1359-1369).
//
// The file (DESIGN.md §4.19 has the definition in full): baseline sequential JPEG as libjpeg writes it for these planes with
// its default, accurate integer DCT - JFIF 1.01 header, Annex K's quantisation bases scaled by the quality, Annex K's four
// Huffman tables, 2x2 luma sampling, one scan, no restart markers.  The reference passes TJFLAG_FASTDCT (hb.c:607), the AAN
// transform, whose rounding nothing here can be held against; container, tables and entropy code are the same and every
// decoder reads both alike.  The arithmetic of a block is csrc/jpeg_block.h, which tools/jpeg_block_check runs on the host.
//
// Six launches per picture on the context's stream, behind the frame's contents (hbhip_frame_use_on).  Whatever one
// workgroup needs of another is a launch boundary: no workgroup waits on another's flag.
//   jpeg_blocks    a thread per block of the scan (MCU raster order, Y00 Y01 Y10 Y11 Cb Cr): the samples by clamped loads
//                  (the plane continued by its last column and row), the transform, quantisation, 64 coefficients in
//                  scan order.  Dummy blocks - luma blocks of an edge MCU beyond ceil(w / 8) x ceil(h / 8) - store nothing.
//   jpeg_code      a thread per block: the DC of the component's previous real block, the block's bit string into its
//                  256-byte slot (at most 1660 bits) and its length; the workgroup's 256 lengths are summed in place
//                  (exclusive) and their total goes to the chunk list.
//   jpeg_scan_top  one workgroup: the exclusive sum of the chunk list (64-bit: 16384 x 16384 of noise passes 2^32 bits).
//   jpeg_pack      a thread per dword of the scan BEFORE stuffing: it finds the block that covers its first bit (two binary
//                  searches: chunks, then the chunk's blocks) and gathers from there on - five blocks and more on flat
//                  content, a fiftieth of one on noise.  No read-modify-write, no zeroed buffer.  The last dword is filled
//                  with ones.  It counts its 0xFF bytes; the workgroup's counts are summed like the lengths.
//   jpeg_scan_top  the same kernel over the 0xFF counts.
//   jpeg_stuff     a thread per dword again: its bytes to where the counts put them, a zero byte behind every 0xFF; the
//                  first thread leaves the record (scan bytes, bits).
// The header (623 bytes) is built once on the host.  A pull waits for the record (16 bytes), then copies exactly the scan's
// bytes behind the header in the caller's buffer and waits for that copy: nothing else crosses the bus.
#include "hbhip_internal.h"
#include "jpeg_block.h"

namespace {

typedef unsigned long long u64;

constexpr int kChunk = 256;                      // blocks of a jpeg_code workgroup, dwords of a jpeg_pack / jpeg_stuff one
constexpr int kHeaderBytes = 623;
constexpr int kSlotWords = JPB_SLOT_BYTES / 4;

struct JpegRecord { u64 scan_bytes, bits; };

struct JpegPlanes
{
    const uint8_t *plane[3];
    int pitch[3];
};

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        const unsigned t = __shfl_up(v, off, 64);
        v += lane >= off ? t : 0u;
    }
    return v;
}

// the exclusive sum of v over the 256 threads of a workgroup; *total: the sum of all (s_wave: 4 entries of LDS)
__device__ __forceinline__ unsigned group_excl_scan(unsigned v, unsigned *s_wave, unsigned *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned inc = wave_incl_scan(v, lane);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++)
    {
        const unsigned s = s_wave[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kChunk) void jpeg_blocks_kernel(JpegPlanes src, JpbGeom g, int nblocks,
                                                              const JpbTables *__restrict__ tables, uint4 *__restrict__ coefs)
{
    const int b = blockIdx.x * kChunk + threadIdx.x;
    if (b >= nblocks) return;
    const JpbPlace p = jpb_place(g, b);
    if (p.dummy) return;
    const int pw = p.comp ? g.width >> 1 : g.width, ph = p.comp ? g.height >> 1 : g.height;
    const uint8_t *plane = p.comp == 0 ? src.plane[0] : p.comp == 1 ? src.plane[1] : src.plane[2];
    const int pitch = p.comp == 0 ? src.pitch[0] : p.comp == 1 ? src.pitch[1] : src.pitch[2];
    int d[64];
    jpb_load_block(plane, pitch, pw, ph, p.bx, p.by, d);
    int16_t zz[64];
    jpb_transform_block(d, tables->divisor[p.comp != 0], zz);
    uint4 *out = coefs + (size_t)b * 8;
#pragma unroll
    for (int q = 0; q < 8; q++)
    {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            w[i] = (unsigned)(uint16_t)zz[8 * q + 2 * i] | ((unsigned)(uint16_t)zz[8 * q + 2 * i + 1] << 16);
        out[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// a block's bits, most significant first, into dwords whose VALUE holds the earlier bit in the higher place; the bits of
// the last dword beyond the string are zero
struct SlotSink
{
    unsigned *slot;
    u64 acc = 0;
    int held = 0, words = 0, bits = 0;
    __device__ __forceinline__ void put(uint32_t code, int n)
    {
        acc = (acc << n) | code;
        held += n; bits += n;
        if (held >= 32)
        {
            held -= 32;
            if (words < kSlotWords) slot[words] = (unsigned)(acc >> held);
            words++;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (held > 0 && words < kSlotWords) slot[words] = (unsigned)(acc << (32 - held));
    }
};

// blk[b] = (bits of the chunk's blocks before b, b's own bits); chunk_bits[blockIdx.x] = the chunk's bits
__global__ __launch_bounds__(kChunk) void jpeg_code_kernel(JpbGeom g, int nblocks, const JpbTables *__restrict__ tables,
                                                            const uint4 *__restrict__ coefs, unsigned *__restrict__ slots,
                                                            uint2 *__restrict__ blk, u64 *__restrict__ chunk_bits)
{
    __shared__ unsigned s_wave[4];
    const int b = blockIdx.x * kChunk + threadIdx.x;
    unsigned len = 0;
    if (b < nblocks)
    {
        const JpbPlace p = jpb_place(g, b);
        const int tb = p.comp != 0;
        SlotSink sink;
        sink.slot = slots + (size_t)b * kSlotWords;
        if (p.dummy)
            jpb_code_dummy(tables->dc[tb], tables->ac[tb], sink);
        else
        {
            const int from = jpb_pred_block(g, b);
            const int pred = from < 0 ? 0 : (int)(int16_t)(reinterpret_cast<const unsigned *>(coefs + (size_t)from * 8)[0] & 0xffffu);
            uint4 v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = coefs[(size_t)b * 8 + q];
            auto coef = [&v](int k) {
                const uint4 q = v[k >> 3];
                const int i = (k >> 1) & 3;
                const unsigned w = i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w;
                return (int)(int16_t)((k & 1 ? w >> 16 : w) & 0xffffu);
            };
            jpb_code_block(coef, pred, tables->dc[tb], tables->ac[tb], sink);
        }
        sink.finish();
        len = (unsigned)sink.bits;
    }
    unsigned total;
    const unsigned before = group_excl_scan(len, s_wave, &total);
    if (b < nblocks) blk[b] = make_uint2(before, len);
    if (threadIdx.x == 0) chunk_bits[blockIdx.x] = total;
}

// x[0 .. n) to its exclusive sum in place, the sum of all to *total.  `bits` given: only the chunks of dwords that a scan of
// *bits bits has (the 0xFF counts: jpeg_pack leaves the chunks behind the scan's end unwritten).
__global__ __launch_bounds__(1024) void jpeg_scan_top_kernel(u64 *__restrict__ x, int n, const u64 *__restrict__ bits,
                                                              u64 *__restrict__ total)
{
    __shared__ u64 s_wave[16];
    if (bits)
    {
        const u64 chunks = ((*bits + 31) / 32 + kChunk - 1) / kChunk;     // (n: never more than the buffers hold)
        if (chunks < (u64)n) n = (int)chunks;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 carry = 0;
    for (int base = 0; base < n; base += 1024)
    {
        const int i = base + tid;
        const u64 v = i < n ? x[i] : 0;
        u64 inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
        {
            const unsigned lo = __shfl_up((unsigned)inc, off, 64), hi = __shfl_up((unsigned)(inc >> 32), off, 64);
            inc += lane >= off ? ((u64)hi << 32 | lo) : 0;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; w++)
        {
            const u64 s = s_wave[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (i < n) x[i] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// 32 bits of a block's string from bit r on (r from -31: the string starts inside the dword); bits outside the string are zero
__device__ __forceinline__ unsigned slot_bits(const unsigned *__restrict__ slot, int len, int r)
{
    const int words = min((len + 31) >> 5, kSlotWords);
    const int wi = r >> 5, sh = r & 31;                           // (arithmetic shift: -1 for a negative r)
    const unsigned hi = wi >= 0 && wi < words ? slot[wi] : 0u;
    const unsigned lo = wi + 1 < words ? slot[wi + 1] : 0u;
    return sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
}

// packed[j]: bits 32 j .. 32 j + 31 of the scan, the earlier bit in the higher place; ff[j]: the 0xFF bytes of the chunk's
// dwords before j; ff_chunk[blockIdx.x]: the chunk's
__global__ __launch_bounds__(kChunk) void jpeg_pack_kernel(int nblocks, int nchunks, u64 max_dwords, const u64 *__restrict__ chunk_bits,
                                                            const u64 *__restrict__ total_bits, const uint2 *__restrict__ blk,
                                                            const unsigned *__restrict__ slots, unsigned *__restrict__ packed,
                                                            uint16_t *__restrict__ ff, u64 *__restrict__ ff_chunk)
{
    __shared__ unsigned s_wave[4];
    const u64 total = min(*total_bits, 32 * max_dwords);          // (what the buffers hold; no scan is longer)
    const u64 ndw = (total + 31) / 32, nbytes = (total + 7) / 8;
    const u64 j = (u64)blockIdx.x * kChunk + threadIdx.x;
    if ((u64)blockIdx.x * kChunk >= ndw) return;                  // (the whole workgroup)
    unsigned count = 0;
    if (j < ndw)
    {
        const u64 pos = 32 * j, end = pos + 32;
        // every block has bits (four at the least), so the starts rise strictly: the last one at or before pos covers it
        int lo = 0, hi = nchunks - 1;
        while (lo < hi)
        {
            const int mid = (lo + hi + 1) >> 1;
            if (chunk_bits[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        const int c = lo;
        const unsigned r = (unsigned)(pos - chunk_bits[c]);
        lo = 0; hi = min(kChunk, nblocks - c * kChunk) - 1;
        while (lo < hi)
        {
            const int mid = (lo + hi + 1) >> 1;
            if (blk[c * kChunk + mid].x <= r) lo = mid; else hi = mid - 1;
        }
        unsigned val = 0;
        for (int b = c * kChunk + lo; b < nblocks; b++)
        {
            const uint2 e = blk[b];
            const u64 start = chunk_bits[b / kChunk] + e.x;
            if (start >= end) break;
            val |= slot_bits(slots + (size_t)b * kSlotWords, (int)e.y, (int)((long long)pos - (long long)start));
        }
        if (j == ndw - 1 && (total & 31)) val |= 0xffffffffu >> (unsigned)(total & 31);   // the last byte's fill, and beyond
        packed[j] = val;
#pragma unroll
        for (int k = 0; k < 4; k++) count += 4 * j + k < nbytes && ((val >> (24 - 8 * k)) & 0xffu) == 0xffu;
    }
    unsigned all;
    const unsigned before = group_excl_scan(count, s_wave, &all);
    if (j < ndw) ff[j] = (uint16_t)before;
    if (threadIdx.x == 0) ff_chunk[blockIdx.x] = all;
}

__global__ __launch_bounds__(kChunk) void jpeg_stuff_kernel(u64 max_dwords, const u64 *__restrict__ total_bits, const unsigned *__restrict__ packed,
                                                             const uint16_t *__restrict__ ff, const u64 *__restrict__ ff_chunk,
                                                             const u64 *__restrict__ ff_total, uint8_t *__restrict__ out,
                                                             JpegRecord *__restrict__ rec)
{
    const u64 total = min(*total_bits, 32 * max_dwords);
    const u64 ndw = (total + 31) / 32, nbytes = (total + 7) / 8;
    const u64 j = (u64)blockIdx.x * kChunk + threadIdx.x;
    if (j == 0) { rec->scan_bytes = nbytes + *ff_total; rec->bits = total; }
    if (j >= ndw) return;
    const unsigned val = packed[j];
    u64 at = 4 * j + ff_chunk[blockIdx.x] + ff[j];
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const unsigned byte = (val >> (24 - 8 * k)) & 0xffu;
        if (4 * j + k < nbytes)
        {
            out[at++] = (uint8_t)byte;
            if (byte == 0xffu) out[at++] = 0;
        }
    }
}

struct Slot
{
    DevBuf<uint8_t> d_out;                       // the record (64 bytes), then the stuffed scan
    JpegRecord  *h_rec = nullptr;
    hipEvent_t   done = nullptr;
    hbhip_frame *frame = nullptr;
};

void put16(std::vector<uint8_t> &v, int x) { v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x); }

void segment(std::vector<uint8_t> &v, int marker, const std::vector<uint8_t> &payload)
{
    v.push_back(0xff); v.push_back((uint8_t)marker);
    put16(v, (int)payload.size() + 2);
    v.insert(v.end(), payload.begin(), payload.end());
}

// SOI, APP0 (JFIF 1.01, density 1 x 1, no unit, no thumbnail), DQT 0, DQT 1, SOF0, DHT 00 10 01 11, SOS: what libjpeg writes
std::vector<uint8_t> jpeg_header(int width, int height, int quality)
{
    std::vector<uint8_t> v = {0xff, 0xd8};
    segment(v, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    constexpr int order[64] = JPB_ZIGZAG;
    for (int c = 0; c < 2; c++)
    {
        uint8_t q[64];
        jpb_quant_table(c, quality, q);
        std::vector<uint8_t> p = {(uint8_t)c};
        for (int k = 0; k < 64; k++) p.push_back(q[order[k]]);
        segment(v, 0xdb, p);
    }
    std::vector<uint8_t> sof = {8};
    put16(sof, height); put16(sof, width);
    for (uint8_t x : {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) sof.push_back(x);
    segment(v, 0xc0, sof);
    for (int id = 0; id < 2; id++)
        for (int cls = 0; cls < 2; cls++)
        {
            const JpbHuffSpec *s = jpb_huff_spec(cls, id);
            std::vector<uint8_t> p = {(uint8_t)(cls << 4 | id)};
            p.insert(p.end(), s->bits, s->bits + 16);
            p.insert(p.end(), s->vals, s->vals + s->nvals);
            segment(v, 0xc4, p);
        }
    segment(v, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return v;
}

} // namespace

struct hbhip_jpeg
{
    hbhip_ctx *ctx = nullptr;
    int width = 0, height = 0, quality = 0;
    JpbGeom geom;
    int nblocks = 0, nchunks = 0;                // blocks of the scan; jpeg_code's workgroups
    size_t max_dwords = 0;                       // of a scan before stuffing: every block at JPB_MAX_BLOCK_BITS
    int npack = 0;                               // jpeg_pack's workgroups for that many
    std::vector<uint8_t> header;
    // What the launches hand on to each other: one set for every picture - the pictures' launches follow each other on
    // the context's stream.  One allocation; only a picture's stuffed scan and record are its slot's own.
    DevBuf<uint8_t> d_work;
    JpbTables *d_tables = nullptr;
    uint4     *d_coefs = nullptr;
    unsigned  *d_slots = nullptr, *d_packed = nullptr;
    uint2     *d_blk = nullptr;
    u64       *d_chunk_bits = nullptr, *d_ff_chunk = nullptr, *d_totals = nullptr;      // d_totals: [0] bits, [1] 0xFF bytes
    uint16_t  *d_ff = nullptr;
    PinnedBuf<JpegRecord> h_recs;                // one per slot
    std::vector<Slot *> slots, idle;
    std::deque<Slot *> inflight;

    ~hbhip_jpeg()
    {
        for (Slot *s : slots)
        {
            if (s->frame) hbhip_frame_release(s->frame);
            if (s->done) (void)hipEventDestroy(s->done);
            delete s;
        }
    }

    size_t scan_bound() const { return 8 * max_dwords; }         // every byte of it 0xFF

    Slot *take_slot()
    {
        if (!idle.empty()) { Slot *s = idle.back(); idle.pop_back(); return s; }
        if ((int)slots.size() >= HBHIP_JPEG_INFLIGHT_MAX) return nullptr;
        Slot *s = new (std::nothrow) Slot;
        if (!s) return nullptr;
        if (s->d_out.alloc(ctx, 64 + scan_bound()) != HBHIP_OK ||
            hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess)
        {
            (void)hipGetLastError();
            delete s;
            return nullptr;
        }
        s->h_rec = h_recs.get() + slots.size();
        slots.push_back(s);
        return s;
    }
};

// what push refuses for the size alone (create asks the same of its own)
static int jpeg_size_check(int width, int height)
{
    if ((width | height) & 1) return HBHIP_ERR_UNSUPPORTED;
    if (width < 8 || height < 8 || width > 16384 || height > 16384) return HBHIP_ERR_UNSUPPORTED;
    return HBHIP_OK;
}

extern "C" int hbhip_jpeg_create(hbhip_ctx *ctx, int width, int height, int quality, hbhip_jpeg **out)
{
    if (!ctx || !out) return HBHIP_ERR_ARG;
    *out = nullptr;
    if (quality < 1 || quality > 100) return HBHIP_ERR_ARG;
    const int rc = jpeg_size_check(width, height);
    if (rc != HBHIP_OK) return rc;
    (void)hipSetDevice(ctx->device);
    hbhip_jpeg *j = new (std::nothrow) hbhip_jpeg;
    if (!j) return HBHIP_ERR_NOMEM;
    j->ctx = ctx; j->width = width; j->height = height; j->quality = quality;
    j->geom = jpb_geom(width, height);
    j->nblocks = 6 * j->geom.mcus_w * j->geom.mcus_h;
    j->nchunks = (j->nblocks + kChunk - 1) / kChunk;
    j->max_dwords = ((size_t)j->nblocks * JPB_MAX_BLOCK_BITS + 31) / 32;
    j->npack = (int)((j->max_dwords + kChunk - 1) / kChunk);
    j->header = jpeg_header(width, height, quality);
    // the work area, every part on a 256-byte boundary
    size_t at = 0;
    auto part = [&at](size_t bytes) { const size_t here = at; at += (bytes + 255) / 256 * 256; return here; };
    const size_t tables_at = part(sizeof(JpbTables)), totals_at = part(2 * sizeof(u64));
    const size_t coefs_at = part((size_t)j->nblocks * 128), slots_at = part((size_t)j->nblocks * JPB_SLOT_BYTES);
    const size_t blk_at = part((size_t)j->nblocks * sizeof(uint2)), chunk_at = part((size_t)j->nchunks * sizeof(u64));
    const size_t packed_at = part(j->max_dwords * 4), ff_at = part(j->max_dwords * 2), ffc_at = part((size_t)j->npack * sizeof(u64));
    int ra = j->d_work.alloc(ctx, at);
    if (ra == HBHIP_OK) ra = j->h_recs.alloc(ctx, HBHIP_JPEG_INFLIGHT_MAX);
    if (ra == HBHIP_OK)
    {
        uint8_t *w = j->d_work.get();
        j->d_tables = reinterpret_cast<JpbTables *>(w + tables_at);
        j->d_totals = reinterpret_cast<u64 *>(w + totals_at);
        j->d_coefs = reinterpret_cast<uint4 *>(w + coefs_at);
        j->d_slots = reinterpret_cast<unsigned *>(w + slots_at);
        j->d_blk = reinterpret_cast<uint2 *>(w + blk_at);
        j->d_chunk_bits = reinterpret_cast<u64 *>(w + chunk_at);
        j->d_packed = reinterpret_cast<unsigned *>(w + packed_at);
        j->d_ff = reinterpret_cast<uint16_t *>(w + ff_at);
        j->d_ff_chunk = reinterpret_cast<u64 *>(w + ffc_at);
        JpbTables t;
        jpb_tables(quality, &t);
        const hipError_t e = hipMemcpy(j->d_tables, &t, sizeof(t), hipMemcpyHostToDevice);
        if (e != hipSuccess) ra = ctx->fail(e, "jpeg: the tables' copy");
        else ctx->bus_h2d += sizeof(t);
    }
    if (ra != HBHIP_OK)
    {
        delete j;
        return ra;
    }
    *out = j;
    return HBHIP_OK;
}

extern "C" void hbhip_jpeg_destroy(hbhip_jpeg *j)
{
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    (void)hipStreamSynchronize(j->ctx->stream);
    delete j;
}

extern "C" size_t hbhip_jpeg_bound(hbhip_jpeg *j)
{
    return j ? kHeaderBytes + j->scan_bound() + 2 : 0;
}

extern "C" int hbhip_jpeg_inflight(hbhip_jpeg *j)
{
    return j ? (int)j->inflight.size() : 0;
}

// the six launches and the record's copy for the picture in `sl`
static int jpeg_queue(hbhip_jpeg *j, Slot *sl, const hbhip_frame *fr)
{
    hbhip_ctx *ctx = j->ctx;
    JpegPlanes src;
    for (int c = 0; c < 3; c++) { src.plane[c] = fr->pic.plane[c]; src.pitch[c] = fr->pic.pitch[c]; }
    JpegRecord *d_rec = reinterpret_cast<JpegRecord *>(sl->d_out.get());
    uint8_t *d_scan = sl->d_out.get() + 64;
    u64 *total_bits = j->d_totals, *total_ff = j->d_totals + 1;
    HBHIP_LAUNCH(ctx, "jpeg_blocks", jpeg_blocks_kernel, dim3(j->nchunks), dim3(kChunk), 0,
                 src, j->geom, j->nblocks, (const JpbTables *)j->d_tables, j->d_coefs);
    HBHIP_LAUNCH(ctx, "jpeg_code", jpeg_code_kernel, dim3(j->nchunks), dim3(kChunk), 0,
                 j->geom, j->nblocks, (const JpbTables *)j->d_tables, (const uint4 *)j->d_coefs, j->d_slots, j->d_blk, j->d_chunk_bits);
    HBHIP_LAUNCH(ctx, "jpeg_scan_top(bits)", jpeg_scan_top_kernel, dim3(1), dim3(1024), 0,
                 j->d_chunk_bits, j->nchunks, (const u64 *)nullptr, total_bits);
    HBHIP_LAUNCH(ctx, "jpeg_pack", jpeg_pack_kernel, dim3(j->npack), dim3(kChunk), 0,
                 j->nblocks, j->nchunks, (u64)j->max_dwords, (const u64 *)j->d_chunk_bits, (const u64 *)total_bits, (const uint2 *)j->d_blk,
                 (const unsigned *)j->d_slots, j->d_packed, j->d_ff, j->d_ff_chunk);
    HBHIP_LAUNCH(ctx, "jpeg_scan_top(0xff)", jpeg_scan_top_kernel, dim3(1), dim3(1024), 0,
                 j->d_ff_chunk, j->npack, (const u64 *)total_bits, total_ff);
    HBHIP_LAUNCH(ctx, "jpeg_stuff", jpeg_stuff_kernel, dim3(j->npack), dim3(kChunk), 0,
                 (u64)j->max_dwords, (const u64 *)total_bits, (const unsigned *)j->d_packed, (const uint16_t *)j->d_ff, (const u64 *)j->d_ff_chunk,
                 (const u64 *)total_ff, d_scan, d_rec);
    HBHIP_CHECK(ctx, hipGetLastError());
    HBHIP_CHECK(ctx, hipMemcpyAsync(sl->h_rec, d_rec, sizeof(JpegRecord), hipMemcpyDeviceToHost, ctx->stream));
    HBHIP_CHECK(ctx, hipEventRecord(sl->done, ctx->stream));
    ctx->bus_d2h += sizeof(JpegRecord);
    return HBHIP_OK;
}

extern "C" int hbhip_jpeg_push(hbhip_jpeg *j, hbhip_frame *fr)
{
    if (!j || !fr) return HBHIP_ERR_ARG;
    if (fr->depth != 8 || fr->lcw != 1 || fr->lch != 1) return HBHIP_ERR_UNSUPPORTED;
    const int size_rc = jpeg_size_check(fr->width, fr->height);
    if (size_rc != HBHIP_OK) return size_rc;
    if (fr->width != j->width || fr->height != j->height) return HBHIP_ERR_UNSUPPORTED;
    hbhip_ctx *ctx = j->ctx;
    if (fr->ctx->device != ctx->device) return HBHIP_ERR_ARG;
    for (int c = 0; c < 3; c++)                                   // (what hbhip_frame_alloc gives: jpb_load_block reads whole dwords)
        if (((uintptr_t)fr->pic.plane[c] & 15) || (fr->pic.pitch[c] & 15) || fr->pic.pitch[c] < hbhip_align_up(fr->pic.width[c], 16))
            return HBHIP_ERR_ARG;
    if ((int)j->inflight.size() >= HBHIP_JPEG_INFLIGHT_MAX) return HBHIP_ERR_STATE;
    (void)hipSetDevice(ctx->device);
    Slot *sl = j->take_slot();
    if (!sl) return HBHIP_ERR_NOMEM;
    int rc = hbhip_frame_use_on(fr, ctx);
    if (rc == HBHIP_OK)
    {
        hbhip_frame_retain(fr);
        rc = jpeg_queue(j, sl, fr);
        if (rc != HBHIP_OK)
        {
            (void)hipStreamSynchronize(ctx->stream);              // whatever was queued reads the frame and the slot
            hbhip_frame_release(fr);
        }
    }
    if (rc != HBHIP_OK)
    {
        j->idle.push_back(sl);
        return rc;
    }
    sl->frame = fr;
    j->inflight.push_back(sl);
    return HBHIP_OK;
}

extern "C" int hbhip_jpeg_pull(hbhip_jpeg *j, uint8_t *dst, size_t cap, size_t *size)
{
    if (!j || !dst || !size) return HBHIP_ERR_ARG;
    *size = 0;
    if (j->inflight.empty()) return HBHIP_AGAIN;
    hbhip_ctx *ctx = j->ctx;
    (void)hipSetDevice(ctx->device);
    Slot *sl = j->inflight.front();
    const hipError_t e = hipEventSynchronize(sl->done);
    j->inflight.pop_front();
    hbhip_frame_release(sl->frame);
    sl->frame = nullptr;
    int rc = e == hipSuccess ? HBHIP_OK : ctx->fail(e, "jpeg: wait for the picture's record");
    if (rc == HBHIP_OK)
    {
        const size_t scan = (size_t)sl->h_rec->scan_bytes;
        *size = kHeaderBytes + scan + 2;
        if (scan > j->scan_bound()) rc = ctx->fail(hipErrorUnknown, "jpeg: the record's length");
        else if (*size > cap) rc = HBHIP_ERR_ARG;                 // the picture is dropped: its slot is free again
        else
        {
            // the record is on the host, so the scan is complete in device memory: its copy needs no order on a stream
            hipStream_t down = ctx->down();
            memcpy(dst, j->header.data(), kHeaderBytes);
            const hipError_t ec = hipMemcpyAsync(dst + kHeaderBytes, sl->d_out.get() + 64, scan, hipMemcpyDeviceToHost, down);
            if (ec != hipSuccess) { (void)hipStreamSynchronize(down); rc = ctx->fail(ec, "jpeg: the scan's copy"); }
            else rc = hbhip_wait_behind(ctx, down, "jpeg: the scan's copy");
            if (rc == HBHIP_OK)
            {
                ctx->bus_d2h += scan;
                dst[kHeaderBytes + scan] = 0xff; dst[kHeaderBytes + scan + 1] = 0xd9;
            }
        }
    }
    j->idle.push_back(sl);
    return rc;
}
