// Interlaced input: the two byte-bound kernels of the deinterlacing loop (include/atmvfi.h, atmvfi_field_bob / atmvfi_field_rows;
// atm-vfi_amd/fields.py holds the definitions, the host twins bob_numpy / rows_numpy and the loop, tests/cpu_fields.py the per-pixel
// models).  Nothing of the reference.
//
// atmvfi_field_bob.  One launch reads the picture of a woven canvas once and writes both field canvases.  With S the picture (h x w at
// (pad_top, pad_left) of the [planes,Hp,Wp] source) and F_p = bob(S, p):
//     F_p[y] = S[y]                          y & 1 == p
//            = S[1]                          y == 0          (else)
//            = S[h - 2]                      y == h - 1
//            = 0.5f * (S[y - 1] + S[y + 1])                  (one rounding: the halving is exact)
//     dst_p[c][Y][X] = F_p[c][clamp(Y - pad_top, 0, h - 1)][clamp(X - pad_left, 0, w - 1)]
// A lane owns four adjacent canvas columns of a strip of ATMVFI_FIELD_BOB_STRIP picture rows and walks down the strip with the previous
// two source rows in registers: a source element is loaded once per strip (strip + 2 row loads for 2 * strip row stores) and feeds the
// real row of one output and the averaged rows of the other.  The loads of eight rows are issued together, ahead of their stores: a lane
// that waited for each row in turn was bound by seventeen memory latencies in a row, not by bytes (README, "Interlaced input").  The
// lane that owns picture row 0 (h - 1) also writes the canvas rows above (below) the picture.  Vector instance (all three pointers 16-byte aligned, Wp, pad_left and w multiples of 4): a column group lies
// whole inside the picture (one 16-byte load) or whole inside the left / right padding (the edge column, one scalar load, broadcast);
// every store is 16 bytes.  Scalar instance: four clamped scalar loads and up to four scalar stores.  The two give the same bits: the
// arithmetic is per element.  The source's padding is never read; every destination element is written by exactly one lane; vector
// stores only, no atomics, nothing pre-zeroed, no LDS.
//
// atmvfi_field_rows.  Rows y = parity (mod 2) of up to three planes from src to dst: bytes, moved.  A plane whose two base addresses,
// two pitches and row_bytes are multiples of 16 moves 16 bytes per lane, any other plane one byte per lane (consecutive lanes,
// consecutive bytes); the geometry travels in the kernel arguments.  Grid-stride, 256 threads.
#include "common.h"

namespace {

constexpr int kStrip = ATMVFI_FIELD_BOB_STRIP;
constexpr int kBatch = 8;          // rows whose loads are issued together
static_assert(kStrip % kBatch == 0, "a strip is whole batches");

struct BobArgs {
    const float* src;
    float* dst[2];          // by parity; either may be null
    int Hp, Wp, pad_top, pad_left, h, w;
    int groups;             // column groups of a canvas row, ceil(Wp / 4)
    int strips;             // ceil(h / kStrip)
    int total;              // planes * strips * groups
};

// the four source values of picture row y under canvas columns X0 .. X0 + 3 (columns clamped into the picture)
template <bool VEC>
__device__ __forceinline__ f32x4 bob_load(const float* plane, const BobArgs& a, int y, int X0) {
    const float* row = plane + (long long)(a.pad_top + y) * a.Wp;
    const int lo = a.pad_left, hi = a.pad_left + a.w - 1;
    if (VEC) {
        if (X0 >= lo && X0 <= hi) return *reinterpret_cast<const f32x4*>(row + X0);      // (w % 4 == 0: the group is whole)
        const float e = row[X0 < lo ? lo : hi];
        return f32x4{e, e, e, e};
    }
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int x = X0 + i;
        x = x < lo ? lo : (x > hi ? hi : x);
        v[i] = row[x];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void bob_store(float* plane, const BobArgs& a, int Y, int X0, const f32x4 v) {
    float* row = plane + (long long)Y * a.Wp + X0;
    if (VEC) {
        *reinterpret_cast<f32x4*>(row) = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (X0 + i < a.Wp) row[i] = v[i];
}

// picture row y of one field canvas, and with it the canvas rows outside the picture that replicate it
template <bool VEC>
__device__ __forceinline__ void bob_emit(float* plane, const BobArgs& a, int y, int X0, const f32x4 v) {
    if (!plane) return;
    bob_store<VEC>(plane, a, a.pad_top + y, X0, v);
    if (y == 0)
        for (int Y = 0; Y < a.pad_top; ++Y) bob_store<VEC>(plane, a, Y, X0, v);
    if (y == a.h - 1)
        for (int Y = a.pad_top + a.h; Y < a.Hp; ++Y) bob_store<VEC>(plane, a, Y, X0, v);
}

template <bool VEC>
__global__ __launch_bounds__(256) void field_bob_kernel(const BobArgs a) {
    const long long plane_elems = (long long)a.Hp * a.Wp;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += gridDim.x * blockDim.x) {
        const int g = idx % a.groups, t = idx / a.groups;
        const int strip = t % a.strips, c = t / a.strips;
        const int X0 = 4 * g, y0 = strip * kStrip;
        const int y1 = y0 + kStrip < a.h ? y0 + kStrip : a.h;
        const float* sp = a.src + c * plane_elems;
        float* d0 = a.dst[0] ? a.dst[0] + c * plane_elems : nullptr;
        float* d1 = a.dst[1] ? a.dst[1] + c * plane_elems : nullptr;
        // the rows above and at the strip's top, then kBatch rows at a time: their loads are independent of one another and of the
        // stores, so a batch is in flight at once (a row index beyond the picture is clamped to its last row: loaded, never used)
        f32x4 up = bob_load<VEC>(sp, a, y0 > 0 ? y0 - 1 : 0, X0);
        f32x4 mid = bob_load<VEC>(sp, a, y0, X0);
        for (int yb = y0; yb < y1; yb += kBatch) {
            f32x4 below[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) below[i] = bob_load<VEC>(sp, a, yb + 1 + i < a.h ? yb + 1 + i : a.h - 1, X0);
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int y = yb + i;
                const f32x4 down = below[i];
                if (y < y1) {
                    // the row of the field that does not own y (h >= 2: row 1 and row h - 2 exist)
                    const f32x4 fill = y == 0 ? down : (y == a.h - 1 ? up : 0.5f * (up + down));
                    const bool odd = (y & 1) != 0;
                    bob_emit<VEC>(odd ? d1 : d0, a, y, X0, mid);
                    bob_emit<VEC>(odd ? d0 : d1, a, y, X0, fill);
                }
                up = mid;
                mid = down;
            }
        }
    }
}

struct RowsPlane {
    long long dst_offset, src_offset, dst_pitch, src_pitch;
    long long units;        // per row: 16-byte pieces (vec) or bytes
    long long first;        // the plane's first work item
    int vec;
    int pad;
};
struct RowsArgs {
    unsigned char* dst;
    const unsigned char* src;
    RowsPlane p[3];
    long long total;
    int planes, parity;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void field_rows_kernel(const RowsArgs a) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (long long)gridDim.x * blockDim.x) {
        int k = 0;
        if (a.planes > 1 && idx >= a.p[1].first) k = 1;
        if (a.planes > 2 && idx >= a.p[2].first) k = 2;
        const RowsPlane& p = a.p[k];
        const long long j = idx - p.first;
        const long long r = j / p.units, u = j - r * p.units;
        const long long y = 2 * r + a.parity;
        unsigned char* d = a.dst + p.dst_offset + y * p.dst_pitch;
        const unsigned char* s = a.src + p.src_offset + y * p.src_pitch;
        if (p.vec) reinterpret_cast<u32x4*>(d)[u] = reinterpret_cast<const u32x4*>(s)[u];
        else d[u] = s[u];
    }
}

inline bool overlap(uintptr_t a0, uintptr_t an, uintptr_t b0, uintptr_t bn) { return a0 < b0 + bn && b0 < a0 + an; }

}  // namespace

extern "C" int atmvfi_field_bob(const float* src, float* dst_even, float* dst_odd, int planes, int Hp, int Wp, int pad_top, int pad_left,
                                int h, int w, void* stream) {
    ATMVFI_REQUIRE(src && (dst_even || dst_odd), ATMVFI_EINVAL, "field_bob: null pointer (src %p, dst_even %p, dst_odd %p: a source and at least one destination)",
                   (const void*)src, (void*)dst_even, (void*)dst_odd);
    ATMVFI_REQUIRE(planes >= 1 && Hp >= 1 && Wp >= 1, ATMVFI_EINVAL, "field_bob: bad shape (planes %d, canvas %d x %d)", planes, Hp, Wp);
    ATMVFI_REQUIRE(h >= 2, ATMVFI_EINVAL, "field_bob: a picture of %d rows has no two fields (h must be at least 2)", h);
    ATMVFI_REQUIRE(w >= 1 && pad_top >= 0 && pad_left >= 0 && (long long)pad_top + h <= Hp && (long long)pad_left + w <= Wp, ATMVFI_EINVAL,
                   "field_bob: window %d x %d at (%d, %d) outside the %d x %d canvas", h, w, pad_top, pad_left, Hp, Wp);
    const long long elems = (long long)planes * Hp * Wp;
    const uintptr_t bytes = (uintptr_t)elems * 4u, s0 = reinterpret_cast<uintptr_t>(src), e0 = reinterpret_cast<uintptr_t>(dst_even),
                    o0 = reinterpret_cast<uintptr_t>(dst_odd);
    ATMVFI_REQUIRE(((s0 | e0 | o0) & 3u) == 0, ATMVFI_EINVAL, "field_bob: pointers must be 4-byte aligned");
    ATMVFI_REQUIRE(!(dst_even && overlap(s0, bytes, e0, bytes)) && !(dst_odd && overlap(s0, bytes, o0, bytes)), ATMVFI_EINVAL,
                   "field_bob: a destination overlaps the source (not in place)");
    ATMVFI_REQUIRE(!(dst_even && dst_odd && overlap(e0, bytes, o0, bytes)), ATMVFI_EINVAL, "field_bob: the two destinations overlap");
    BobArgs a = {src, {dst_even, dst_odd}, Hp, Wp, pad_top, pad_left, h, w, (Wp + 3) / 4, (h + kStrip - 1) / kStrip, 0};
    const long long total = (long long)planes * a.strips * a.groups;
    ATMVFI_REQUIRE(total < (1ll << 30), ATMVFI_EINVAL, "field_bob: %d planes of %d x %d are too large (the work-item count must fit an int)", planes, Hp, Wp);
    a.total = (int)total;
    const bool vec = atmvfi::aligned16(src) && (!dst_even || atmvfi::aligned16(dst_even)) && (!dst_odd || atmvfi::aligned16(dst_odd)) &&
                     Wp % 4 == 0 && pad_left % 4 == 0 && w % 4 == 0;
    const dim3 grid(grid_for(total));
    if (vec) hipLaunchKernelGGL((field_bob_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((field_bob_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("field_bob");
}

extern "C" int atmvfi_field_rows(void* dst, const void* src, int planes, const int64_t* geometry, int parity, void* stream) {
    ATMVFI_REQUIRE(dst && src && geometry, ATMVFI_EINVAL, "field_rows: null pointer (dst %p, src %p, geometry %p)", dst, src, (const void*)geometry);
    ATMVFI_REQUIRE(planes >= 1 && planes <= 3, ATMVFI_EINVAL, "field_rows: bad plane count %d (1..3)", planes);
    ATMVFI_REQUIRE(parity == 0 || parity == 1, ATMVFI_EINVAL, "field_rows: bad parity %d (0: the even rows, 1: the odd rows)", parity);
    RowsArgs a = {};
    a.dst = (unsigned char*)dst, a.src = (const unsigned char*)src, a.planes = planes, a.parity = parity;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), s0 = reinterpret_cast<uintptr_t>(src);
    uintptr_t db[3], dn[3], sb[3], sn[3];       // the byte ranges a plane's rows span, as written and as read
    long long total = 0;
    for (int k = 0; k < planes; ++k) {
        const int64_t* g = geometry + 6 * k;
        const long long doff = g[0], soff = g[1], dp = g[2], sp = g[3], rb = g[4], rows = g[5];
        ATMVFI_REQUIRE(doff >= 0 && soff >= 0 && dp >= 1 && sp >= 1 && rb >= 1 && rows >= 1 && rows < (1ll << 31) && dp < (1ll << 40) && sp < (1ll << 40) &&
                           doff < (1ll << 46) && soff < (1ll << 46),
                       ATMVFI_EINVAL, "field_rows: bad geometry of plane %d (offsets %lld / %lld, pitches %lld / %lld, row_bytes %lld, rows %lld)", k, doff, soff, dp,
                       sp, rb, rows);
        ATMVFI_REQUIRE(rb <= dp && rb <= sp, ATMVFI_EINVAL, "field_rows: row_bytes %lld of plane %d above a pitch (dst %lld, src %lld)", rb, k, dp, sp);
        const long long n = (rows - parity + 1) / 2;           // the rows of this parity
        const long long last = n > 0 ? 2 * (n - 1) + parity : 0;
        db[k] = d0 + (uintptr_t)(doff + parity * dp), dn[k] = n > 0 ? (uintptr_t)((last - parity) * dp + rb) : 0;
        sb[k] = s0 + (uintptr_t)(soff + parity * sp), sn[k] = n > 0 ? (uintptr_t)((last - parity) * sp + rb) : 0;
        RowsPlane& p = a.p[k];
        p.dst_offset = doff, p.src_offset = soff, p.dst_pitch = dp, p.src_pitch = sp;
        p.vec = ((d0 + (uintptr_t)doff) % 16 == 0 && (s0 + (uintptr_t)soff) % 16 == 0 && dp % 16 == 0 && sp % 16 == 0 && rb % 16 == 0) ? 1 : 0;
        p.units = p.vec ? rb / 16 : rb;
        p.first = total;
        total += n * p.units;
        ATMVFI_REQUIRE(total < (1ll << 40), ATMVFI_EINVAL, "field_rows: the planes are too large");
    }
    for (int k = 0; k < planes; ++k) {
        if (!dn[k]) continue;
        for (int j = 0; j < planes; ++j) {
            ATMVFI_REQUIRE(!(sn[j] && overlap(db[k], dn[k], sb[j], sn[j])), ATMVFI_EINVAL, "field_rows: the rows written of plane %d overlap the rows read of plane %d",
                           k, j);
            ATMVFI_REQUIRE(!(j > k && dn[j] && overlap(db[k], dn[k], db[j], dn[j])), ATMVFI_EINVAL, "field_rows: the rows written of planes %d and %d overlap", k, j);
        }
    }
    if (total == 0) return ATMVFI_OK;           // (every plane has one row and the parity is 1)
    a.total = total;
    hipLaunchKernelGGL(field_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("field_rows");
}
