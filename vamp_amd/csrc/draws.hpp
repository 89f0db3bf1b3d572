// draws.hpp -- the stretch move's counter-based draws: Philox4x32-10 (Salmon et al., SC'11), the keyed red/blue split
// of every chunk of walkers (DESIGN.md "red/blue split") and the draws of one mover.  The kernels of libvamp_hip.so
// (k_draws, k_half_step, k_run_resident, k_scatter_rows) and the host implementation of the same C ABI
// (oracle/vamp_cpu.cpp) both draw through these functions, so the two follow the same trajectories.  The scatter of
// walker-sharded runs states draw_move's slot -> walker map itself (k_scatter_rows, vamp_cpu.cpp's scatter_part): a
// shared form changed the kernel's generated code.  The tests check both libraries against an independent Python
// restatement of the draws.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define VAMP_DRAW_HD __host__ __device__ __forceinline__
#else
#define VAMP_DRAW_HD inline
#endif

namespace vamp {

struct U4 { unsigned c0, c1, c2, c3; };
VAMP_DRAW_HD U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c.c0;
        const unsigned long long p1 = 0xCD9E8D57ull * c.c2;
        U4 n;
        n.c0 = (unsigned)(p1 >> 32) ^ c.c1 ^ k0;
        n.c1 = (unsigned)p1;
        n.c2 = (unsigned)(p0 >> 32) ^ c.c3 ^ k1;
        n.c3 = (unsigned)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
VAMP_DRAW_HD double u53(unsigned hi, unsigned lo) {
    return (double)((((unsigned long long)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}
// high 64 bits of the 128-bit product
VAMP_DRAW_HD unsigned long long mul64hi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}
constexpr unsigned STREAM_MOVE = 0, STREAM_ACCEPT = 1, STREAM_SPLIT = 2;

// keyed bijection of [0, block): affine-multiply / xorshift rounds on the next power of two,
// cycle-walking back into range
VAMP_DRAW_HD unsigned split_perm(unsigned long long seed, unsigned step, unsigned chunk, unsigned region, unsigned slot,
                                 unsigned block) {
    const U4 r = philox4x32_10({chunk, step, STREAM_SPLIT, region}, (unsigned)seed, (unsigned)(seed >> 32));
    int bits = 32 - __builtin_clz((block - 1) | 1u);
    if (bits < 1) bits = 1;
    const unsigned long long mask = (1ull << bits) - 1ull;
    int sh = bits / 2;
    if (sh < 1) sh = 1;
    const unsigned long long m0 = ((unsigned long long)r.c0 << 1) | 1ull, m2 = ((unsigned long long)r.c2 << 1) | 1ull;
    unsigned long long v = slot;
    for (;;) {
        v = (v * m0 + r.c1) & mask;  v ^= v >> sh;
        v = (v * m2 + r.c3) & mask;  v ^= v >> sh;
        v = (v * 0x9E3779B1ull + (r.c0 ^ r.c3)) & mask;  v ^= v >> sh;
        if (v < block) return (unsigned)v;
    }
}

// Sampler: the sampler's scalars W (walkers per region), split_block, a (stretch scale) and seed, and region_rng_id(S, r),
// region r's identity in the draw keys (vamp_set_region_ids) -- SamplerDev on the device, vamp::AbiState on the host.
// The draws read them where they first need them: read earlier, they change the kernels' generated code.

// The draws of one mover: which walker holds active slot `a_loc` of `region` in this (step, half) -- position
// a_loc % (block / 2) in the half of chunk a_loc / (block / 2) that moves --, its stretch factor, its partner from the frozen colour and log(u2) for the accept test.
struct MoveDraw { long long ws, wc; double z, logu; };
template <class Sampler>
VAMP_DRAW_HD MoveDraw draw_move(const Sampler& S, unsigned step, int half, int region, long long a_loc) {
    const long long halfW = S.W >> 1;
    const unsigned hb = (unsigned)(S.split_block >> 1);
    const unsigned chunk = (unsigned)(a_loc / hb);
    const unsigned pos = (unsigned)(a_loc % hb);
    MoveDraw d;
    // draws are keyed by the region's rng_id, not by its position in the context: a region follows the same
    // trajectory whichever device (and whichever subset of a spectrum's regions) holds it
    const unsigned rid = (unsigned)region_rng_id(S, region);
    d.ws = (long long)chunk * S.split_block +
           split_perm(S.seed, step, chunk, rid, pos + (half ? hb : 0u), (unsigned)S.split_block);
    const long long gid = (long long)rid * S.W + d.ws;
    const unsigned k0 = (unsigned)S.seed, k1 = (unsigned)(S.seed >> 32);
    const U4 r = philox4x32_10({(unsigned)gid, step, ((unsigned)half << 8) | STREAM_MOVE, (unsigned)(gid >> 32)}, k0, k1);
    const double u1 = u53(r.c0, r.c1);
    const double t = (S.a - 1.0) * u1 + 1.0;
    d.z = t * t / S.a;
    const unsigned long long j = mul64hi(((unsigned long long)r.c2 << 32) | r.c3, (unsigned long long)halfW);
    const unsigned cchunk = (unsigned)(j / hb);
    const unsigned cpos = (unsigned)(j % hb);
    d.wc = (long long)cchunk * S.split_block +
           split_perm(S.seed, step, cchunk, rid, cpos + (half ? 0u : hb), (unsigned)S.split_block);
    const U4 r2 = philox4x32_10({(unsigned)gid, step, ((unsigned)half << 8) | STREAM_ACCEPT, (unsigned)(gid >> 32)}, k0, k1);
    const double u2 = u53(r2.c0, r2.c1);
    d.logu = u2 > 0.0 ? log(u2) : -__builtin_huge_val();
    return d;
}

}  // namespace vamp
