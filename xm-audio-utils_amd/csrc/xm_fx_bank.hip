// xm_fx_bank.hip — the comb bank (include/xm_effects.h, effect kind 4) for
// gfx950: N feedback combs in parallel on one input, summed in a fixed order.
//
//   c_k[i] = b0_k*x[i] + (bd_k*x[i-Ds_k] - ad_k*c_k[i-Ds_k]),  Ds_k = D_k * channels
//   y[i]   = ((dry*x[i] + mix_0*c_0[i]) + mix_1*c_1[i]) + ...
//
// every operation a separately rounded fp32 op (-ffp-contract=off).
//
// One workgroup of 1024 lanes owns one clip at a time and walks it in time
// blocks of BL = min(min_k Ds_k, XMH_BANK_BLOCK) samples.  Inside a block every
// x[i-Ds_k] and c_k[i-Ds_k] lies in an earlier block, so all positions of all
// branches are independent: lane t takes positions t and t + 1024 of the
// block, one barrier separates two blocks.  The clip is read once and written
// once; a sample is read and written by the same lane, so in == out is safe.
//
// Delay lines (the "rings") of the clip: branch k's outputs in a ring of Ds_k
// samples, sample i at slot i mod Ds_k: the lane reads c_k[i-Ds_k] from the
// slot it then writes c_k[i] to, consecutive lanes consecutive slots (unit
// stride, conflict-free).  The inputs in a ring of R = max Ds + XMH_BANK_BLOCK
// samples, sample i at slot (i + max Ds) mod R: the block reads samples
// [t0 - max Ds, t0) and writes [t0, t0 + BL), which never share a slot.  The
// input ring is kept for every bank: in place the clip's own x is overwritten,
// and a product bd*x[i-Ds] is formed even for bd = 0 (its zero's sign is part
// of the contract).  Slots are tracked by per-branch block bases (wave-uniform,
// one conditional subtract per block), never by a division.
//
// Placement (template RL): rings of up to XMH_BANK_LDS_FLOATS samples in LDS
// (dynamic, up to the CU's whole 160 KiB); longer ones in a slot of device
// scratch per workgroup (job.bank_scratch), same body, global accesses.
//
// The x loads do not depend on the recurrence: a lane keeps BK_U blocks of its
// positions in flight in registers (global-address loads, so the compiler's
// waits are counted).  With rings in LDS the barrier is lgkmcnt-only and the
// loads survive it; with rings in scratch every wave drains its stores before
// the barrier so that the next block's readers see them.
#include <stdlib.h>
#include <algorithm>
#include "xm_device.h"

namespace {

constexpr int BK_NT = 1024;                   // lanes of a workgroup
constexpr int BK_P = XMH_BANK_BLOCK / BK_NT;  // positions of a block per lane
constexpr int BK_U = 4;                       // blocks in flight per lane (2048 lanes x 8 dwords = 32 KiB per CU)

template <bool RL> struct BankRing;
template <> struct BankRing<true> { typedef __attribute__((address_space(3))) float T; };
template <> struct BankRing<false> { typedef __attribute__((address_space(1))) float T; };

template <bool RL>
XM_DEV void bank_sync()
{
    if (!RL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // ring stores of this wave have reached the CU's L1 / L2
    __syncthreads();
}

// BK_N: the branches the kernel is unrolled for (4 or 8, bank_n <= BK_N): the
// per-branch constants of a bank of up to four then fit the scalar registers
template <bool RL, bool ST, int BK_N>
__global__ __launch_bounds__(BK_NT) void k_bank(XmhFxJob j)
{
    extern __shared__ float bank_lds[];
    typedef const __attribute__((address_space(1))) float gcf;
    typedef __attribute__((address_space(1))) float gf;
    typedef typename BankRing<RL>::T rf;
    const int tid = threadIdx.x;
    const int nb = j.bank_n;
    const float dry = j.bank_dry;
    // wave-uniform per-branch constants; the k loops are unrolled over BK_N with
    // a k < nb guard, so these arrays are indexed statically (SGPRs, no scratch)
    int Ds[BK_N], roff[BK_N];
    int sum = 0, dmax = 0, dmin = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < BK_N; ++k) {
        Ds[k] = roff[k] = 0;
        if (k < nb) {
            Ds[k] = (int)(j.bank_taps[k].delay * j.channels);
            roff[k] = sum;
            sum += Ds[k];
            dmax = Ds[k] > dmax ? Ds[k] : dmax;
            dmin = Ds[k] < dmin ? Ds[k] : dmin;
        }
    }
    const int R = dmax + XMH_BANK_BLOCK;         // the input ring
    const int H = sum + dmax;                    // streaming history of a clip
    const int BL = dmin < XMH_BANK_BLOCK ? dmin : XMH_BANK_BLOCK;
    const int64_t n = j.frames * j.channels;
    const int64_t nblk = (n + BL - 1) / BL;
    rf *ring = RL ? (rf *)bank_lds : (rf *)(j.bank_scratch + (int64_t)blockIdx.x * (sum + R));
    rf *xring = ring + sum;

    for (int clip = blockIdx.x; clip < j.n_clips; clip += gridDim.x) {
        gcf *x = (gcf *)j.in_ptrs[clip];
        gf *y = (gf *)j.out_ptrs[clip];
        // the rings before the clip: zero, or the carried history (branch k's
        // last Ds_k outputs at slots 0 .. Ds_k-1, the last dmax inputs at
        // slots 0 .. dmax-1 of the input ring: the history's own layout)
        for (int i = tid; i < H; i += BK_NT) ring[i] = ST ? ((gcf *)j.bank_hist_in)[(int64_t)clip * H + i] : 0.0f;
        // block bases: slot of the block's first sample in branch k's ring and
        // in the input ring (x[i - Ds_k] sits Ds_k slots before x[i])
        int cb[BK_N], xw = dmax;
#pragma unroll
        for (int k = 0; k < BK_N; ++k) cb[k] = 0;
        // a lane's positions of block b, loaded unconditionally (indices
        // clamped into the clip: positions past the block or the clip are
        // loaded and never used)
        float xq[BK_U][BK_P];
        auto load = [&](float (&v)[BK_P], int64_t b) {
#pragma unroll
            for (int m = 0; m < BK_P; ++m) {
                int64_t i = b * BL + tid + m * BK_NT;
                i = i < n ? i : n - 1;
                v[m] = x[i];
            }
        };
        // one block.  A slot is base + off wrapped once: min(s, s - size) as
        // unsigned picks s - size exactly when s >= size (and min(s, s + size)
        // picks s + size exactly when s < 0).  A whole block of
        // XMH_BANK_BLOCK samples (the common case: lags of 2048 samples and
        // more) gives every lane all its positions, so nothing is guarded and
        // the positions' arithmetic runs side by side (packed fp32 ops).
        auto step = [&](const float (&v)[BK_P], int64_t b) {
            const int64_t t0 = b * BL;
            const int bl = n - t0 < BL ? (int)(n - t0) : BL;
            const bool whole = bl == XMH_BANK_BLOCK;   // wave-uniform
            float acc[BK_P];
            unsigned sw[BK_P];   // slot of x[i] in the input ring
#pragma unroll
            for (int m = 0; m < BK_P; ++m) {
                acc[m] = dry * v[m];
                sw[m] = xw + tid + m * BK_NT;
                sw[m] = min(sw[m], sw[m] - (unsigned)R);
            }
#pragma unroll
            for (int k = 0; k < BK_N; ++k) {
                if (k < nb) {
                    const float b0 = j.bank_taps[k].b0, bd = j.bank_taps[k].bd, ad = j.bank_taps[k].ad,
                                mix = j.bank_taps[k].mix;
                    rf *rk = ring + roff[k];
                    unsigned sc[BK_P], sx[BK_P];
#pragma unroll
                    for (int m = 0; m < BK_P; ++m) {
                        const unsigned off = tid + m * BK_NT;
                        sc[m] = cb[k] + off;
                        sc[m] = min(sc[m], sc[m] - (unsigned)Ds[k]);
                        sx[m] = sw[m] - (unsigned)Ds[k];   // in (-R, R)
                        sx[m] = min(sx[m], sx[m] + (unsigned)R);
                    }
                    if (whole) {
                        float xd[BK_P], cp[BK_P], c[BK_P];
#pragma unroll
                        for (int m = 0; m < BK_P; ++m) {
                            xd[m] = xring[sx[m]];
                            cp[m] = rk[sc[m]];
                        }
#pragma unroll
                        for (int m = 0; m < BK_P; ++m) {
                            const float p = b0 * v[m], q = bd * xd[m], r = ad * cp[m];
                            const float t = q - r;
                            c[m] = p + t;
                            const float mm = mix * c[m];
                            acc[m] = acc[m] + mm;
                        }
#pragma unroll
                        for (int m = 0; m < BK_P; ++m) rk[sc[m]] = c[m];
                    } else {
#pragma unroll
                        for (int m = 0; m < BK_P; ++m) {
                            if (tid + m * BK_NT < bl) {
                                const float p = b0 * v[m], q = bd * xring[sx[m]], r = ad * rk[sc[m]];
                                const float t = q - r;
                                const float c = p + t;
                                rk[sc[m]] = c;
                                const float mm = mix * c;
                                acc[m] = acc[m] + mm;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < BK_P; ++m) {
                const unsigned off = tid + m * BK_NT;
                if (whole || (int)off < bl) {
                    xring[sw[m]] = v[m];
                    y[t0 + off] = acc[m];
                }
            }
#pragma unroll
            for (int k = 0; k < BK_N; ++k) {
                cb[k] += BL;
                cb[k] = cb[k] >= Ds[k] ? cb[k] - Ds[k] : cb[k];   // BL <= Ds_k
            }
            xw += BL;
            xw = xw >= R ? xw - R : xw;
            bank_sync<RL>();
        };
#pragma unroll
        for (int u = 0; u < BK_U; ++u) load(xq[u], u < nblk ? u : 0);
        bank_sync<RL>();   // the rings are initialised
        for (int64_t b0 = 0; b0 < nblk; b0 += BK_U) {
            if (b0 + 2 * BK_U <= nblk) {
                // a whole round with a whole round to load: straight-line code
#pragma unroll
                for (int u = 0; u < BK_U; ++u) {
                    float v[BK_P];
#pragma unroll
                    for (int m = 0; m < BK_P; ++m) v[m] = xq[u][m];
                    load(xq[u], b0 + u + BK_U);
                    step(v, b0 + u);
                }
            } else {
#pragma unroll
                for (int u = 0; u < BK_U; ++u) {
                    if (b0 + u < nblk) {
                        float v[BK_P];
#pragma unroll
                        for (int m = 0; m < BK_P; ++m) v[m] = xq[u][m];
                        if (b0 + u + BK_U < nblk) load(xq[u], b0 + u + BK_U);
                        step(v, b0 + u);
                    }
                }
            }
        }
        if (ST) {
            // the history after the block, oldest first: sample n - Ds_k + q
            // of c_k sits at slot (n + q) mod Ds_k, sample n - dmax + q of x at
            // slot (n + q) mod R (a line the block did not fill keeps the
            // older history there)
            gf *ho = (gf *)j.bank_hist_out + (int64_t)clip * H;
#pragma unroll
            for (int k = 0; k < BK_N; ++k) {
                if (k < nb) {
                    const int sh = (int)(n % Ds[k]);
                    for (int q = tid; q < Ds[k]; q += BK_NT) {
                        int s = sh + q;
                        s = s >= Ds[k] ? s - Ds[k] : s;
                        ho[roff[k] + q] = ring[roff[k] + s];
                    }
                }
            }
            const int shx = (int)(n % R);
            for (int q = tid; q < dmax; q += BK_NT) {
                int s = shx + q;
                s = s >= R ? s - R : s;
                ho[sum + q] = xring[s];
            }
        }
        bank_sync<RL>();   // the next clip's initialisation overwrites the rings
    }
}

}  // namespace

extern "C" int xmg_launch_fx_bank(const XmhFxJob *j, void *stream)
{
    if (j->bank_n < 1 || j->bank_n > XMH_MAX_BANK || (j->channels != 1 && j->channels != 2)) return -22;
    for (int k = 0; k < j->bank_n; ++k)
        if (j->bank_taps[k].delay < 1 || j->bank_taps[k].delay > (1 << 20)) return -22;
    if (!j->bank_hist_in != !j->bank_hist_out || (j->bank_hist_in && j->bank_hist_in == j->bank_hist_out)) return -22;
    if (j->n_clips == 0 || j->frames == 0) return 0;
    const int64_t ring = xmh_bank_ring_floats(j);
    const bool st = j->bank_hist_in != nullptr;
    const int cus = std::max(1, xmg_cu_count());
    if (ring <= XMH_BANK_LDS_FLOATS) {
        const int bytes = (int)ring * (int)sizeof(float);
        auto k = j->bank_n <= 4 ? (st ? k_bank<true, true, 4> : k_bank<true, false, 4>)
                                : (st ? k_bank<true, true, 8> : k_bank<true, false, 8>);
        const int rc = xmg_func_lds((const void *)k, bytes);
        if (rc) return rc;
        // two workgroups per CU fit (lanes: 2 x 1024) while each needs half the LDS at most
        const int per_cu = 2 * bytes <= XMH_BANK_LDS_FLOATS * (int)sizeof(float) ? 2 : 1;
        const unsigned grid = (unsigned)std::min<int64_t>(j->n_clips, (int64_t)cus * per_cu);
        hipLaunchKernelGGL(k, dim3(grid), dim3(BK_NT), (size_t)bytes, (hipStream_t)stream, *j);
        return hipGetLastError() == hipSuccess ? 0 : -1001;
    }
    if (!j->bank_scratch || j->bank_scratch_slots < 1) return -22;
    auto k = j->bank_n <= 4 ? (st ? k_bank<false, true, 4> : k_bank<false, false, 4>)
                            : (st ? k_bank<false, true, 8> : k_bank<false, false, 8>);
    const unsigned grid =
        (unsigned)std::min<int64_t>(j->n_clips, std::min<int64_t>(j->bank_scratch_slots, (int64_t)cus * 2));
    hipLaunchKernelGGL(k, dim3(grid), dim3(BK_NT), 0, (hipStream_t)stream, *j);
    return hipGetLastError() == hipSuccess ? 0 : -1001;
}
