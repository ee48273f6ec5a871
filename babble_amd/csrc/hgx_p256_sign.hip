// Batched ECDSA P-256 signing and public-key derivation: Event.Sign
// (hashgraph/event.go:129-140) = crypto.Sign (crypto/utils.go:37-39) for a batch of digests, one lane
// per signature, with RFC 6979 nonces (hgx_p256_sign_dev.h), and d G for a batch of private keys. Both
// read the base point's comb table (the verify path's table slot nk).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hgx.h"
#include "hgx_kernels.h"
#include "hgx_p256_sign_dev.h"

namespace hgx {

using namespace p256;

// one lane per (key index, digest): R and S as 32 big-endian bytes each. priv32 rows are private keys
// in [1, N-1] and key_idx is in range (the callers checked both on the host).
__global__ void __launch_bounds__(kSignBlock) k_p256_sign(int64_t count, const int32_t* __restrict__ key_idx,
                                                          const uint8_t* __restrict__ priv32,
                                                          const uint8_t* __restrict__ dig,
                                                          const uint32_t* __restrict__ tg, uint8_t* __restrict__ out_r,
                                                          uint8_t* __restrict__ out_s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fe d, e, r, s;
    load_be_words(d, priv32 + 32 * (int64_t)key_idx[i]);
    load_be_words(e, dig + 32 * i);
    p256_sign_one(r, s, d, e, tg);
    store_be(out_r + 32 * i, r);
    store_be(out_s + 32 * i, s);
}

// one lane per private key (in [1, N-1], or all zero: the row is then left as it is): 0x04 | X | Y of d G
__global__ void __launch_bounds__(kSignBlock) k_p256_pub(int nk, const uint8_t* __restrict__ priv32,
                                                         const uint32_t* __restrict__ tg, uint8_t* __restrict__ out65) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nk) return;
    Fe d;
    load_be_words(d, priv32 + 32 * (int64_t)i);
    if (is_zero(d)) return;
    Pt acc;
    comb_mul_g(acc, d, tg);
    Fe zi, zi2, zi3, t, x, y;
    mpow_m2<ModP>(zi, acc.Z, kPm2, kOneP);
    mmul<ModP>(zi2, zi, zi);
    mmul<ModP>(zi3, zi2, zi);
    Fe one = {1, 0, 0, 0, 0, 0, 0, 0};
    mmul<ModP>(t, acc.X, zi2);
    mmul<ModP>(x, t, one);
    mmul<ModP>(t, acc.Y, zi3);
    mmul<ModP>(y, t, one);
    uint8_t* o = out65 + 65 * (int64_t)i;   // (rows of 65 bytes: bytewise)
    o[0] = 0x04;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t a = x[7 - j], b = y[7 - j];
        o[1 + 4 * j] = (uint8_t)(a >> 24); o[2 + 4 * j] = (uint8_t)(a >> 16);
        o[3 + 4 * j] = (uint8_t)(a >> 8); o[4 + 4 * j] = (uint8_t)a;
        o[33 + 4 * j] = (uint8_t)(b >> 24); o[34 + 4 * j] = (uint8_t)(b >> 16);
        o[35 + 4 * j] = (uint8_t)(b >> 8); o[36 + 4 * j] = (uint8_t)b;
    }
}

void launch_p256_sign(hipStream_t s, int64_t count, const int32_t* key_idx, const uint8_t* priv32, const uint8_t* dig,
                      const uint32_t* tab_g, uint8_t* out_r, uint8_t* out_s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_p256_sign, dim3((unsigned)((count + kSignBlock - 1) / kSignBlock)), dim3(kSignBlock), 0, s,
                       count, key_idx, priv32, dig, tab_g, out_r, out_s);
}

void launch_p256_pub(hipStream_t s, int nk, const uint8_t* priv32, const uint32_t* tab_g, uint8_t* out65) {
    if (nk <= 0) return;
    hipLaunchKernelGGL(k_p256_pub, dim3((unsigned)((nk + kSignBlock - 1) / kSignBlock)), dim3(kSignBlock), 0, s, nk,
                       priv32, tab_g, out65);
}

// 1 <= d < N for a 32-byte big-endian d
bool p256_scalar_ok(const uint8_t* d32) {
    static const uint8_t kN[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,
                                   0xBC, 0xE6, 0xFA, 0xAD, 0xA7, 0x17, 0x9E, 0x84, 0xF3, 0xB9, 0xCA, 0xC2, 0xFC, 0x63, 0x25, 0x51};
    bool zero = true;
    for (int j = 0; j < 32; j++) zero = zero && d32[j] == 0;
    return !zero && std::memcmp(d32, kN, 32) < 0;
}

}  // namespace hgx

namespace {

void sign_err(hgx_error* err, int32_t code, const char* msg) {
    if (!err) return;
    err->code = code;
    std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
}

bool sign_gfx950(int32_t device) {
    int ndev = 0;
    hipDeviceProp_t prop;
    return hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev &&
           hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// device copies of one call: the private keys (zeroed before they are freed), G's table, the batch
struct SignRun {
    uint8_t *priv = nullptr, *dig = nullptr, *r = nullptr, *s = nullptr, *valid = nullptr, *pub = nullptr;
    int32_t* idx = nullptr;
    uint32_t* tab = nullptr;
    size_t priv_bytes = 0;
    hipStream_t st = nullptr;
    ~SignRun() {
        if (priv && st) {
            (void)hipMemsetAsync(priv, 0, priv_bytes, st);
            (void)hipStreamSynchronize(st);
        }
        for (void* q : {(void*)priv, (void*)dig, (void*)r, (void*)s, (void*)valid, (void*)pub, (void*)idx, (void*)tab})
            if (q) (void)hipFree(q);
        if (st) (void)hipStreamDestroy(st);
    }
    hipError_t keys(const uint8_t* priv32, int32_t nk) {
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        priv_bytes = 32 * (size_t)nk;
        if (e == hipSuccess) e = hipMalloc((void**)&priv, priv_bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&valid, 1);
        if (e == hipSuccess) e = hipMalloc((void**)&tab, hgx::p256_table_bytes(0));
        if (e == hipSuccess) e = hipMemcpyAsync(priv, priv32, priv_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hgx::launch_p256_tables(st, 0, nullptr, tab, valid);   // no keys: the base point's table alone
            e = hipGetLastError();
        }
        return e;
    }
};

const char* keys_bad(const uint8_t* priv32, int32_t n_keys) {
    if (!priv32 || n_keys <= 0) return "bad arguments";
    for (int32_t k = 0; k < n_keys; k++)
        if (!hgx::p256_scalar_ok(priv32 + 32 * (size_t)k)) return "a private key is 0 or not below N";
    return nullptr;
}

}  // namespace

extern "C" int32_t hgx_p256_sign_batch(int32_t device, const uint8_t* priv32, int32_t n_keys, const int32_t* key_idx,
                                       const uint8_t* digest32, int64_t count, uint8_t* out_r32, uint8_t* out_s32,
                                       hgx_error* err) {
    sign_err(err, HGX_OK, "");
    auto bad = [&](const char* why) {
        char msg[160];
        std::snprintf(msg, sizeof(msg), "hgx_p256_sign_batch: %s", why);
        sign_err(err, HGX_ERR_INVALID, msg);
        return (int32_t)HGX_ERR_INVALID;
    };
    if (count < 0 || count > (int64_t)UINT32_MAX * 64 || (count > 0 && (!key_idx || !digest32 || !out_r32 || !out_s32)))
        return bad("bad arguments");
    if (const char* why = keys_bad(priv32, n_keys)) return bad(why);
    for (int64_t i = 0; i < count; i++)
        if (key_idx[i] < 0 || key_idx[i] >= n_keys) return bad("a key index is outside [0, n_keys)");
    if (count == 0) return HGX_OK;
    if (!sign_gfx950(device)) {
        sign_err(err, HGX_ERR_DEVICE, "no gfx950 (MI355X) HIP device (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipError_t e;
    {
        SignRun run;
        e = run.keys(priv32, n_keys);
        if (e == hipSuccess) e = hipMalloc((void**)&run.idx, 4 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&run.dig, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&run.r, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMalloc((void**)&run.s, 32 * (size_t)count);
        if (e == hipSuccess) e = hipMemcpyAsync(run.idx, key_idx, 4 * (size_t)count, hipMemcpyHostToDevice, run.st);
        if (e == hipSuccess) e = hipMemcpyAsync(run.dig, digest32, 32 * (size_t)count, hipMemcpyHostToDevice, run.st);
        if (e == hipSuccess) {
            hgx::launch_p256_sign(run.st, count, run.idx, run.priv, run.dig, run.tab, run.r, run.s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_r32, run.r, 32 * (size_t)count, hipMemcpyDeviceToHost, run.st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_s32, run.s, 32 * (size_t)count, hipMemcpyDeviceToHost, run.st);
        if (e == hipSuccess) e = hipStreamSynchronize(run.st);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        sign_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    return HGX_OK;
}

extern "C" int32_t hgx_p256_public_keys(int32_t device, const uint8_t* priv32, int32_t n_keys, uint8_t* out_keys65,
                                        hgx_error* err) {
    sign_err(err, HGX_OK, "");
    const char* why = !out_keys65 ? "bad arguments" : keys_bad(priv32, n_keys);
    if (why) {
        char msg[160];
        std::snprintf(msg, sizeof(msg), "hgx_p256_public_keys: %s", why);
        sign_err(err, HGX_ERR_INVALID, msg);
        return HGX_ERR_INVALID;
    }
    if (!sign_gfx950(device)) {
        sign_err(err, HGX_ERR_DEVICE, "no gfx950 (MI355X) HIP device (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipError_t e;
    {
        SignRun run;
        e = run.keys(priv32, n_keys);
        if (e == hipSuccess) e = hipMalloc((void**)&run.pub, 65 * (size_t)n_keys);
        if (e == hipSuccess) {
            hgx::launch_p256_pub(run.st, n_keys, run.priv, run.tab, run.pub);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_keys65, run.pub, 65 * (size_t)n_keys, hipMemcpyDeviceToHost, run.st);
        if (e == hipSuccess) e = hipStreamSynchronize(run.st);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        sign_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    return HGX_OK;
}
