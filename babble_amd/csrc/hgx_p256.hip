// Batched ECDSA P-256 signature verification: Event.Verify (hashgraph/event.go:142-152) =
// crypto.Verify (crypto/utils.go:41-43) = Go's ecdsa.Verify on elliptic.P256() for every
// event of a sync batch, one lane per signature.
//
//   r, s in [1, N-1]; e = digest (32 bytes, big-endian; e mod N); w = s^-1 mod N;
//   u1 = e w, u2 = r w (mod N); (X : Y : Z) = u1 G + u2 Q; valid iff Z != 0 and
//   X / Z^2 == r (mod N).
//
// Arithmetic (hgx_p256_dev.h, shared with the signer): 8 x 32-bit limbs, Montgomery multiplication (CIOS, v_mad_u64_u32) modulo p
// (field) and modulo N (scalars, s^-1 by Fermat); Jacobian points, a = -3 doubling
// (dbl-2001-b) and complete-case addition (add-2007-bl, doubling / infinity branches per
// lane). u1 G + u2 Q by fixed-base combs: for G and for every key (a context has few, each
// signing many events) a table of b * 256^j * P for the 32 byte positions j and the 255 digits b,
// affine, built once when the keys are set (512 KB per key, hgx_set_participant_keys); a verify is
// then at most 64 mixed Jacobian + affine additions (madd-2007-bl, 7M + 4S) and no doubling. The
// final compare avoids the field inversion: X == r Z^2 or, when r + N < p, X == (r + N) Z^2.
// Public keys that are not P-256 points (Go's elliptic.Unmarshal returns nil) give 2.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hgx.h"
#include "hgx_kernels.h"
#include "hgx_p256_dev.h"

namespace hgx {

using namespace p256;

// Tables, step 1: one thread per (key, byte position j): P_j = 256^j P (8 j doublings of the key's
// point), Jacobian, into base[key][j]; thread j = 0 also checks the key (0x04 prefix, X, Y < p,
// Y^2 = X^3 - 3X + b) into valid[key]. Key nk is the base point G.
__global__ void __launch_bounds__(64) k_p256_comb_base(int nk, const uint8_t* __restrict__ keys65,
                                                       uint32_t* __restrict__ base, uint8_t* __restrict__ valid) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = t / kCombPos, j = t % kCombPos;
    if (k > nk) return;
    Fe x, y;
    bool ok = true;
    if (k < nk) {
        const uint8_t* q = keys65 + 65 * (size_t)k;
        ok = q[0] == 0x04;
        load_be(x, q + 1);
        load_be(y, q + 33);
        ok = ok && lt(x, ModP::n) && lt(y, ModP::n);
    } else {
        cpy(x, kGx);
        cpy(y, kGy);
    }
    Pt P;
    mmul<ModP>(P.X, x, kR2P);
    mmul<ModP>(P.Y, y, kR2P);
    cpy(P.Z, kOneP);
    if (ok) {   // on the curve: y^2 == x^3 - 3x + b
        Fe l, r, tt;
        mmul<ModP>(l, P.Y, P.Y);
        mmul<ModP>(tt, P.X, P.X);
        mmul<ModP>(r, tt, P.X);
        msub<ModP>(r, r, P.X);
        msub<ModP>(r, r, P.X);
        msub<ModP>(r, r, P.X);
        madd<ModP>(r, r, kBm);
        ok = eq(l, r);
    }
    if (j == 0) valid[k] = ok ? 1 : 0;
    if (!ok) return;
    for (int d = 0; d < 8 * j; d++) {
        Pt t2;
        pdbl(t2, P);
        P = t2;
    }
    uint32_t* o = base + ((size_t)k * kCombPos + j) * 24;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        o[q] = P.X[q];
        o[8 + q] = P.Y[q];
        o[16 + q] = P.Z[q];
    }
}

// Tables, step 2: one thread per (key, j, digit b in [1, 255]): b P_j by double-and-add over b's
// bits, to affine (Z^-1 by Fermat). A valid key's point has prime order, so no b P_j (b < 256, P_j
// != O) is the point at infinity.
__global__ void __launch_bounds__(64) k_p256_comb_fill(int nk, const uint32_t* __restrict__ base,
                                                       const uint8_t* __restrict__ valid, uint32_t* __restrict__ tab) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = 1 + (int)(t % 255);
    const int64_t kj = t / 255;
    const int k = (int)(kj / kCombPos), j = (int)(kj % kCombPos);
    if (k > nk || !valid[k]) return;
    Pt Pj;
    const uint32_t* bp = base + ((size_t)k * kCombPos + j) * 24;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        Pj.X[q] = bp[q];
        Pj.Y[q] = bp[8 + q];
        Pj.Z[q] = bp[16 + q];
    }
    Pt acc = Pj;
    const int top = 31 - __builtin_clz((unsigned)b);
    for (int bit = top - 1; bit >= 0; bit--) {
        Pt t2;
        pdbl(t2, acc);
        acc = t2;
        if ((b >> bit) & 1) {
            padd(t2, acc, Pj);
            acc = t2;
        }
    }
    Fe zi, zi2, tt;
    mpow_m2<ModP>(zi, acc.Z, kPm2, kOneP);
    mmul<ModP>(zi2, zi, zi);
    uint32_t* e = tab + (size_t)k * kTabWords + ((size_t)j * kCombDig + b) * kEntWords;
    mmul<ModP>(tt, acc.X, zi2);
#pragma unroll
    for (int q = 0; q < 8; q++) e[q] = tt[q];
    mmul<ModP>(tt, zi2, zi);
    mmul<ModP>(zi, acc.Y, tt);
#pragma unroll
    for (int q = 0; q < 8; q++) e[8 + q] = zi[q];
}


__global__ void __launch_bounds__(128) k_p256_verify(int64_t count, int nk, const int32_t* __restrict__ key_idx,
                                                     const uint8_t* __restrict__ dig,
                                                     const uint8_t* __restrict__ rr, const uint8_t* __restrict__ ss,
                                                     const uint32_t* __restrict__ tab,
                                                     const uint8_t* __restrict__ valid, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int k = key_idx[i];
    if (k < 0 || k >= nk || !valid[k]) {
        out[i] = 2;
        return;
    }
    Fe r, s, e;
    load_be(r, rr + 32 * i);
    load_be(s, ss + 32 * i);
    load_be(e, dig + 32 * i);
    if (is_zero(r) || is_zero(s) || !lt(r, ModN::n) || !lt(s, ModN::n)) {
        out[i] = 0;
        return;
    }
    if (!lt(e, ModN::n)) {   // e < 2^256 < 2N: one subtraction
        Fe z = {0, 0, 0, 0, 0, 0, 0, 0};
        madd<ModN>(e, e, z);
    }
    // w = s^-1 (Montgomery form), by s^(N-2)
    Fe sm, w, u1, u2;
    mmul<ModN>(sm, s, kR2N);
    mpow_m2<ModN>(w, sm, kNm2, kOneN);
    mmul<ModN>(u1, e, w);   // e s^-1 (plain form)
    mmul<ModN>(u2, r, w);
    // fixed-base combs for G and for the key: u1 G + u2 Q = sum over the 32 byte positions j of
    // T_G[j][u1 byte j] + T_Q[j][u2 byte j], at most 64 mixed additions and no doubling; the next
    // position's two entries are loaded while the current ones are added
    const uint32_t* __restrict__ tg = tab + (size_t)nk * kTabWords;
    const uint32_t* __restrict__ tq = tab + (size_t)k * kTabWords;
    Pt acc;
#pragma unroll
    for (int q = 0; q < 8; q++) { acc.X[q] = 0; acc.Y[q] = 0; acc.Z[q] = 0; }
    Fe gx, gy, qx, qy;
    uint32_t d1 = u1[0] & 255u, d2 = u2[0] & 255u;
    ent_load(gx, gy, tg + (size_t)d1 * kEntWords);
    ent_load(qx, qy, tq + (size_t)d2 * kEntWords);
    for (int j = 0; j < kCombPos; j++) {
        Fe ngx, ngy, nqx, nqy;
        uint32_t n1 = 0, n2 = 0;
        if (j + 1 < kCombPos) {
            n1 = byte_at(u1, j + 1);
            n2 = byte_at(u2, j + 1);
            ent_load(ngx, ngy, tg + ((size_t)(j + 1) * kCombDig + n1) * kEntWords);
            ent_load(nqx, nqy, tq + ((size_t)(j + 1) * kCombDig + n2) * kEntWords);
        }
        if (d1) {
            Pt nx;
            pmadd(nx, acc, gx, gy);
            acc = nx;
        }
        if (d2) {
            Pt nx;
            pmadd(nx, acc, qx, qy);
            acc = nx;
        }
        d1 = n1;
        d2 = n2;
        cpy(gx, ngx); cpy(gy, ngy); cpy(qx, nqx); cpy(qy, nqy);
    }
    if (is_zero(acc.Z)) {
        out[i] = 0;
        return;
    }
    // X == r Z^2, or X == (r + N) Z^2 when r + N < p (x mod N == r, x in [0, p))
    Fe z2, rm, t;
    mmul<ModP>(z2, acc.Z, acc.Z);
    mmul<ModP>(rm, r, kR2P);
    mmul<ModP>(t, rm, z2);
    bool ok = eq(t, acc.X);
    if (!ok) {
        Fe rn;
        uint64_t c = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            c += (uint64_t)r[q] + ModN::n[q];
            rn[q] = (uint32_t)c;
            c >>= 32;
        }
        if (c == 0 && lt(rn, ModP::n)) {
            mmul<ModP>(rm, rn, kR2P);
            mmul<ModP>(t, rm, z2);
            ok = eq(t, acc.X);
        }
    }
    out[i] = ok ? 1 : 0;
}

// the comb tables plus the per-(key, position) base points of step 1 after them
size_t p256_table_bytes(int nk) { return (size_t)(nk + 1) * (kTabWords + (size_t)kCombPos * 24) * 4; }

void launch_p256_tables(hipStream_t s, int nk, const uint8_t* keys65, uint32_t* tab, uint8_t* valid) {
    uint32_t* base = tab + (size_t)(nk + 1) * kTabWords;
    hipLaunchKernelGGL(k_p256_comb_base, dim3(((nk + 1) * kCombPos + 63) / 64), dim3(64), 0, s, nk, keys65, base, valid);
    const int64_t ent = (int64_t)(nk + 1) * kCombPos * 255;
    hipLaunchKernelGGL(k_p256_comb_fill, dim3((unsigned)((ent + 63) / 64)), dim3(64), 0, s, nk, (const uint32_t*)base,
                       (const uint8_t*)valid, tab);
}

void launch_p256_verify(hipStream_t s, int64_t count, int nk, const int32_t* key_idx, const uint8_t* dig,
                        const uint8_t* r, const uint8_t* sg, const uint32_t* tab, const uint8_t* valid, uint8_t* out) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_p256_verify, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, s, count, nk, key_idx, dig,
                       r, sg, tab, valid, out);
}

}  // namespace hgx

namespace {

void p256_err(hgx_error* err, int32_t code, const char* msg) {
    if (!err) return;
    err->code = code;
    std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
}

bool gfx950(int32_t device) {
    int ndev = 0;
    hipDeviceProp_t prop;
    return hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev &&
           hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// device copies of a batch: the key tables, then verify launches (the last one's results kept)
struct P256Run {
    uint8_t *keys = nullptr, *dig = nullptr, *r = nullptr, *s = nullptr, *valid = nullptr, *out = nullptr;
    int32_t* idx = nullptr;
    uint32_t* tab = nullptr;
    hipStream_t st = nullptr;
    ~P256Run() {
        for (void* q : {(void*)keys, (void*)dig, (void*)r, (void*)s, (void*)valid, (void*)out, (void*)idx, (void*)tab})
            if (q) (void)hipFree(q);
        if (st) (void)hipStreamDestroy(st);
    }
    hipError_t upload(const uint8_t* k65, int32_t nk, const int32_t* ki, const uint8_t* d, const uint8_t* rr,
                      const uint8_t* ss, int64_t count) {
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void**)&keys, 65 * (size_t)nk + 1);
        if (e == hipSuccess) e = hipMalloc((void**)&idx, 4 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&dig, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&r, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&s, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&out, (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&valid, (size_t)nk + 1);
        if (e == hipSuccess) e = hipMalloc((void**)&tab, hgx::p256_table_bytes(nk));
        if (e == hipSuccess && nk) e = hipMemcpyAsync(keys, k65, 65 * (size_t)nk, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(idx, ki, 4 * (size_t)count, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dig, d, 32 * (size_t)count, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(r, rr, 32 * (size_t)count, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(s, ss, 32 * (size_t)count, hipMemcpyHostToDevice, st);
        return e;
    }
    hipError_t tables(int32_t nk) {
        hgx::launch_p256_tables(st, nk, keys, tab, valid);
        return hipGetLastError();
    }
    hipError_t verify(int32_t nk, int64_t count) {
        hgx::launch_p256_verify(st, count, nk, idx, dig, r, s, tab, valid, out);
        return hipGetLastError();
    }
};

bool p256_args_ok(const uint8_t* keys65, int32_t n_keys, const int32_t* key_idx, const uint8_t* digest,
                  const uint8_t* r, const uint8_t* s, int64_t count, const uint8_t* out) {
    return n_keys >= 0 && count >= 0 && count <= (int64_t)UINT32_MAX * 128 &&
           (n_keys == 0 || keys65) && (count == 0 || (key_idx && digest && r && s && out));
}

}  // namespace

extern "C" int32_t hgx_p256_verify_batch(int32_t device, const uint8_t* keys65, int32_t n_keys, const int32_t* key_idx,
                                         const uint8_t* digest32, const uint8_t* r32, const uint8_t* s32, int64_t count,
                                         uint8_t* out, hgx_error* err) {
    p256_err(err, HGX_OK, "");
    if (!p256_args_ok(keys65, n_keys, key_idx, digest32, r32, s32, count, out)) {
        p256_err(err, HGX_ERR_INVALID, "hgx_p256_verify_batch: bad arguments");
        return HGX_ERR_INVALID;
    }
    if (count == 0) return HGX_OK;
    if (!gfx950(device)) {
        p256_err(err, HGX_ERR_DEVICE, "no gfx950 (MI355X) HIP device (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipError_t e;
    {
        P256Run run;
        e = run.upload(keys65, n_keys, key_idx, digest32, r32, s32, count);
        if (e == hipSuccess) e = run.tables(n_keys);
        if (e == hipSuccess) e = run.verify(n_keys, count);
        if (e == hipSuccess) e = hipMemcpyAsync(out, run.out, (size_t)count, hipMemcpyDeviceToHost, run.st);
        if (e == hipSuccess) e = hipStreamSynchronize(run.st);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        p256_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    return HGX_OK;
}

extern "C" int32_t hgx_p256_verify_bench(int32_t device, const uint8_t* keys65, int32_t n_keys,
                                         const int32_t* key_idx, const uint8_t* digest32, const uint8_t* r32,
                                         const uint8_t* s32, int64_t count, int32_t warmup, int32_t iters,
                                         uint8_t* out, double* ms_per_launch) {
    if (!p256_args_ok(keys65, n_keys, key_idx, digest32, r32, s32, count, out) || count == 0 || iters <= 0 ||
        warmup < 0 || !ms_per_launch)
        return HGX_ERR_INVALID;
    if (!gfx950(device)) return HGX_ERR_DEVICE;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipError_t e;
    float ms = 0.f;
    {
        P256Run run;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        e = run.upload(keys65, n_keys, key_idx, digest32, r32, s32, count);
        if (e == hipSuccess) e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        // the key tables once (a context builds them when its keys are set), then verify launches
        if (e == hipSuccess) e = run.tables(n_keys);
        for (int32_t k = 0; e == hipSuccess && k < warmup; k++) e = run.verify(n_keys, count);
        if (e == hipSuccess) e = hipEventRecord(e0, run.st);
        for (int32_t k = 0; e == hipSuccess && k < iters; k++) e = run.verify(n_keys, count);
        if (e == hipSuccess) e = hipEventRecord(e1, run.st);
        if (e == hipSuccess) e = hipMemcpyAsync(out, run.out, (size_t)count, hipMemcpyDeviceToHost, run.st);
        if (e == hipSuccess) e = hipStreamSynchronize(run.st);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return HGX_ERR_DEVICE;
    *ms_per_launch = (double)ms / iters;
    return HGX_OK;
}
