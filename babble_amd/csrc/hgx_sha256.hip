// Batched SHA-256 of event wire bodies (ingest front end).
//
// The reference hashes one event at a time on the insert path:
//   crypto.SHA256                 crypto/utils.go:11-16
//   Event.Hash  = SHA256(Marshal) hashgraph/event.go:171-180 (the event id, Hex() at :183-188)
//   EventBody.Hash                hashgraph/event.go:48-54   (the bytes Verify checks, :142-152)
//   Block.Hash                    hashgraph/block.go:44-53
// Here a whole batch of already-encoded messages is hashed in one launch: one lane per
// message. The compression and the aligned-load block reader are hgx_sha256_dev.h's (shared
// with the event-body front end, hgx_goenc_dev.hip); what a load may touch around a message
// is stated there and, for the device entry, in include/hgx.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <cstdio>
#include <vector>

#include "hgx.h"
#include "hgx_sha256_dev.h"

namespace hgx {

// One lane per message i = data[offsets[i], offsets[i+1]); digest to out + 32 i.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_sha256_batch(const uint8_t* __restrict__ data,
                                                      const int64_t* __restrict__ offsets, int64_t count,
                                                      uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t off = offsets[i];
    sha256_message<false>(data, off, offsets[i + 1] - off, 0, (uint32_t*)(out + 32 * i));
}


__device__ __host__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// synthetic message bytes for the bench leg: 8 bytes j*8.. = splitmix64(seed + j), little-endian
__global__ void k_fill_bytes(uint64_t* __restrict__ p, int64_t words, uint64_t seed) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < words; j += (int64_t)gridDim.x * blockDim.x)
        p[j] = splitmix64(seed + (uint64_t)j);
}

}  // namespace hgx

namespace {

void set_err(hgx_error* err, int32_t code, const char* msg) {
    if (!err) return;
    err->code = code;
    std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
}

hipError_t launch_sha256(const uint8_t* d_data, const int64_t* d_offsets, int64_t count, uint8_t* d_out,
                         hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(hgx::k_sha256_batch, dim3((unsigned)blocks), dim3(256), 0, s, d_data, d_offsets, count, d_out);
    return hipGetLastError();
}

}  // namespace

extern "C" int32_t hgx_sha256_batch(int32_t device, const uint8_t* data, const int64_t* offsets, int64_t count,
                                    uint8_t* out32, hgx_error* err) {
    set_err(err, HGX_OK, "");
    if (count < 0 || (count > 0 && (!offsets || !out32)) || count > (int64_t)UINT32_MAX * 256) {
        set_err(err, HGX_ERR_INVALID, "hgx_sha256_batch: bad arguments");
        return HGX_ERR_INVALID;
    }
    if (count == 0) return HGX_OK;
    if (offsets[0] < 0) {
        set_err(err, HGX_ERR_INVALID, "hgx_sha256_batch: negative offset");
        return HGX_ERR_INVALID;
    }
    for (int64_t i = 0; i < count; i++)
        if (offsets[i + 1] < offsets[i]) {
            set_err(err, HGX_ERR_INVALID, "hgx_sha256_batch: offsets must be non-decreasing");
            return HGX_ERR_INVALID;
        }
    const int64_t total = offsets[count];
    if (total > 0 && !data) {
        set_err(err, HGX_ERR_INVALID, "hgx_sha256_batch: null data");
        return HGX_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(err, HGX_ERR_DEVICE, "no HIP device available (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (device < 0 || device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(err, HGX_ERR_DEVICE, "libhgx is built for gfx950 (MI355X) only");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    uint8_t *d_data = nullptr, *d_out = nullptr;
    int64_t* d_off = nullptr;
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&d_data, (size_t)total + 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_off, sizeof(int64_t) * (size_t)(count + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, 32 * (size_t)count);
    if (e == hipSuccess && total > 0) e = hipMemcpyAsync(d_data, data, (size_t)total, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (size_t)(count + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_sha256(d_data, d_off, count, d_out, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out32, d_out, 32 * (size_t)count, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (d_data) (void)hipFree(d_data);
    if (d_off) (void)hipFree(d_off);
    if (d_out) (void)hipFree(d_out);
    if (s) (void)hipStreamDestroy(s);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        set_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    return HGX_OK;
}

extern "C" int32_t hgx_sha256_batch_device(const uint8_t* d_data, const int64_t* d_offsets, int64_t count,
                                           uint8_t* d_out32, void* stream) {
    if (count < 0 || (count > 0 && (!d_data || !d_offsets || !d_out32)) || ((uintptr_t)d_out32 & 3))
        return HGX_ERR_INVALID;
    return launch_sha256(d_data, d_offsets, count, d_out32, (hipStream_t)stream) == hipSuccess ? HGX_OK
                                                                                                : HGX_ERR_DEVICE;
}

// Measurement entry for bench.py (no torch on the device side): `count` synthetic messages,
// resident in HBM, hashed warmup + iters times; ms_per_launch from HIP events on the launch stream. Message i has length
// min_len + splitmix64(~seed + i) % (max_len - min_len + 1); the packed bytes are
// splitmix64(seed + j) for 8-byte word j. The digests of the first n_sample messages are
// copied to sample32 so the caller can check them.
extern "C" int32_t hgx_sha256_bench(int32_t device, int64_t count, int32_t min_len, int32_t max_len, uint64_t seed,
                                    int32_t warmup, int32_t iters, double* ms_per_launch, int64_t* total_bytes,
                                    int64_t* n_blocks, int64_t n_sample, uint8_t* sample32) {
    if (count <= 0 || min_len < 0 || max_len < min_len || iters <= 0 || warmup < 0 || n_sample < 0 ||
        n_sample > count || (n_sample && !sample32) || !ms_per_launch)
        return HGX_ERR_INVALID;
    std::vector<int64_t> off((size_t)count + 1);
    int64_t blocks = 0;
    off[0] = 0;
    const uint64_t span = (uint64_t)(max_len - min_len) + 1;
    for (int64_t i = 0; i < count; i++) {
        const int64_t len = min_len + (int64_t)(hgx::splitmix64(~seed + (uint64_t)i) % span);
        off[i + 1] = off[i] + len;
        blocks += (len + 72) >> 6;
    }
    const int64_t total = off[count];
    const int64_t words = (total + 7) / 8 + 1;
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) return HGX_ERR_DEVICE;
    uint8_t *d_data = nullptr, *d_out = nullptr;
    int64_t* d_off = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMalloc((void**)&d_data, (size_t)words * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&d_off, sizeof(int64_t) * (size_t)(count + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, 32 * (size_t)count);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * (size_t)(count + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hgx::k_fill_bytes, dim3(4096), dim3(256), 0, s, (uint64_t*)d_data, words, seed);
        e = hipGetLastError();
    }
    for (int32_t k = 0; e == hipSuccess && k < warmup; k++) e = launch_sha256(d_data, d_off, count, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    for (int32_t k = 0; e == hipSuccess && k < iters; k++) e = launch_sha256(d_data, d_off, count, d_out, s);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess && n_sample) e = hipMemcpyAsync(sample32, d_out, 32 * (size_t)n_sample, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (d_data) (void)hipFree(d_data);
    if (d_off) (void)hipFree(d_off);
    if (d_out) (void)hipFree(d_out);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return HGX_ERR_DEVICE;
    *ms_per_launch = (double)ms / iters;
    if (total_bytes) *total_bytes = total;
    if (n_blocks) *n_blocks = blocks;
    return HGX_OK;
}
