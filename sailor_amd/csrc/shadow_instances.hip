// The per-instance SSBO of a shadow pass, built on the device: FrameGraph/ShadowPrepassNode.cpp:155-201 copies, proxy by proxy on the host, the
// `gpuMatricesData` run of every batch (ShadowPrepassNode::PerInstanceData { mat4 model; }, 64 bytes) into the pass's `data` binding.  Here a batch's run
// is selected by a bitmask over the scene's 96-byte PerInstanceData records -- the layout sailor_hip_csm_caster_masks / sailor_host_csm_plan_passes use,
// LSB first -- and gathered by a kernel:  out[j] = instances[i].model for the j-th set bit i of [begin, end), in ascending i.
//
// Order is by index, never by arrival: a job's bit range is cut into chunks of 1 024 bits,
//   k_shadow_gather_scan  one 1 024-thread block per job: a thread counts one chunk's set bits (popcount over its mask words), the block scans the
//                         counts (shuffle scan in the wave, wave totals through LDS, a carry from tile to tile) and leaves every chunk's exclusive
//                         offset in the workspace and the job's total in its count word;
//   k_shadow_gather       one 256-thread block per chunk: four ballots of 256 bits, mbcnt ranks and the wave totals give every set bit its place in
//                         the chunk (as k4_draw_compact does for 256 records), the places go to LDS as a list of source indices, and the block then
//                         writes its run as ONE linear float4 stream -- four lanes per matrix, so a wave's store covers 1 KiB of consecutive bytes and
//                         its load sixteen 64-byte pieces at a 96-byte stride.
// Jobs (passes x batches) travel by value in the kernel arguments, SG_GROUP at a time: nothing is uploaded, read back or waited for.
// Nothing is written past a job's capacity; its count word still gets the full count.
#include "common.h"

#define SG_CHUNK 1024u        // bits per chunk = four ballots of a 256-thread block
#define SG_THREADS 256u
#define SG_GROUP 32u          // jobs per launch pair (1 280 bytes of jobs + 132 of chunk bases in the kernel arguments)
#define SG_REC4 6u            // float4 per 96-byte SailorPerInstanceData; the model matrix is the first four

struct SgGroup {
    SailorShadowGatherJob job[SG_GROUP];
    uint32_t chunkBase[SG_GROUP + 1]; // first chunk of job j among the group's chunks
};

static inline uint32_t sg_chunks(const SailorShadowGatherJob& j) { return j.end > j.begin ? (j.end - j.begin + SG_CHUNK - 1) / SG_CHUNK : 0u; }

// set bits of [lo, hi), hi > lo, over 32-bit words (the 64-bit words of the mask, little endian)
__device__ __forceinline__ uint32_t sg_popcount_range(const uint32_t* __restrict__ m, uint32_t lo, uint32_t hi)
{
    const uint32_t w0 = lo >> 5, w1 = (hi - 1) >> 5;
    uint32_t n = 0;
    for (uint32_t w = w0; w <= w1; w++) {
        uint32_t v = m[w];
        if (w == w0) v &= 0xFFFFFFFFu << (lo & 31);
        if (w == w1) v &= 0xFFFFFFFFu >> (31 - ((hi - 1) & 31));
        n += (uint32_t)__popc(v);
    }
    return n;
}

__global__ __launch_bounds__(1024) void k_shadow_gather_scan(const SgGroup g, uint32_t* __restrict__ chunkOffset)
{
    __shared__ uint32_t sWave[16];
    __shared__ uint32_t sCarry;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SailorShadowGatherJob job = g.job[blockIdx.x];
    const uint32_t base = g.chunkBase[blockIdx.x], numChunks = g.chunkBase[blockIdx.x + 1] - base;
    const uint32_t* m = (const uint32_t*)job.dMask;
    if (threadIdx.x == 0) sCarry = 0;
    __syncthreads();
    for (uint32_t tile = 0; tile < numChunks; tile += 1024) {
        const uint32_t c = tile + threadIdx.x;
        uint32_t count = 0;
        if (c < numChunks) {
            const uint32_t lo = job.begin + c * SG_CHUNK;
            count = sg_popcount_range(m, lo, min(lo + SG_CHUNK, job.end));
        }
        uint32_t incl = count; // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = sCarry;
        for (uint32_t w = 0; w < wave; w++) before += sWave[w];
        if (c < numChunks) chunkOffset[base + c] = before + incl - count;
        __syncthreads();
        if (threadIdx.x == 1023) sCarry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *job.dCount = sCarry;
}

__global__ __launch_bounds__(SG_THREADS) void k_shadow_gather(const float4* __restrict__ inst, const SgGroup g, const uint32_t numJobs,
                                                              const uint32_t* __restrict__ chunkOffset)
{
    __shared__ uint16_t sMap[SG_CHUNK];
    __shared__ uint32_t sCount[16];   // [ballot s][wave]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t j = 0;
    while (j + 1 < numJobs && g.chunkBase[j + 1] <= blockIdx.x) j++;   // (block-uniform; empty jobs share their successor's base and are passed over)
    const SailorShadowGatherJob job = g.job[j];
    const uint32_t first = job.begin + (blockIdx.x - g.chunkBase[j]) * SG_CHUNK;
    const uint32_t* m = (const uint32_t*)job.dMask;

    bool set[4];
    uint32_t rank[4];
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t i = first + s * SG_THREADS + tid;
        set[s] = i < job.end && ((m[i >> 5] >> (i & 31)) & 1u) != 0u;   // bits at or past `end` do not exist
        const unsigned long long ballot = __ballot(set[s]);
        rank[s] = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
        if (lane == 0) sCount[s * 4 + wave] = (uint32_t)__popcll(ballot);
    }
    __syncthreads();
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            if (w == wave && set[s]) sMap[kept + rank[s]] = (uint16_t)(s * SG_THREADS + tid);
            kept += sCount[s * 4 + w];
        }
    }
    if (kept == 0) return;                                               // (block-uniform)
    __syncthreads();
    const uint32_t dstBase = chunkOffset[blockIdx.x];
    const uint32_t room = job.capacity > dstBase ? min(kept, job.capacity - dstBase) : 0u;
    const uint32_t out4 = room * 4;
    const float4* src = inst + (size_t)first * SG_REC4;
    float4* dst = (float4*)job.dOut + (size_t)dstBase * 4;
    for (uint32_t q0 = 0; q0 < out4; q0 += 4 * SG_THREADS) {             // four requests in flight per lane
        const uint32_t qa = q0 + tid, qb = qa + SG_THREADS, qc = qb + SG_THREADS, qd = qc + SG_THREADS;
        float4 a, b, c, d;   // (four names, not an array: an array indexed in an unrolled loop is promoted to LDS, 16 KiB of it)
        if (qa < out4) a = src[(size_t)sMap[qa >> 2] * SG_REC4 + (qa & 3)];
        if (qb < out4) b = src[(size_t)sMap[qb >> 2] * SG_REC4 + (qb & 3)];
        if (qc < out4) c = src[(size_t)sMap[qc >> 2] * SG_REC4 + (qc & 3)];
        if (qd < out4) d = src[(size_t)sMap[qd >> 2] * SG_REC4 + (qd & 3)];
        if (qa < out4) dst[qa] = a;
        if (qb < out4) dst[qb] = b;
        if (qc < out4) dst[qc] = c;
        if (qd < out4) dst[qd] = d;
    }
}

// ShadowCaster.shader reads inPosition alone out of the mesh's 72-byte vertices; sailor_hip_raster_depth takes packed vec3 positions.  One thread per float:
// the writes are one linear stream, the reads three floats out of every 72 bytes (position at byte 8: texcoord comes first in SailorVertexP3N3T3B3UV2C4).
__global__ __launch_bounds__(256) void k_shadow_positions(const float* __restrict__ vertices, uint32_t numFloats, float* __restrict__ positions)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= numFloats) return;
    const uint32_t v = i / 3u, c = i - 3u * v;
    positions[i] = vertices[(size_t)v * (sizeof(SailorVertexP3N3T3B3UV2C4) / 4) + 2u + c];
}

extern "C" {

int sailor_hip_shadow_extract_positions(SailorHipContext* ctx, const SailorVertexP3N3T3B3UV2C4* dVertices, uint32_t numVertices, float* dPositions)
{
    if (!ctx || numVertices > 0x40000000u || (numVertices != 0 && (!dVertices || !dPositions)) || ((uintptr_t)dVertices & 3) || ((uintptr_t)dPositions & 3))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (numVertices == 0) return SAILOR_HIP_OK;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t numFloats = 3u * numVertices;
    sailor_launch(ctx, k_shadow_positions, dim3((numFloats + 255u) / 256u), dim3(256), (const float*)dVertices, numFloats, dPositions);
    SAILOR_CHECK_LAUNCH(ctx, "k_shadow_positions");
    return SAILOR_HIP_OK;
}

size_t sailor_hip_shadow_gather_workspace_bytes(const SailorShadowGatherJob* jobs, uint32_t numJobs)
{
    size_t chunks = 0;
    for (uint32_t j = 0; jobs && j < numJobs; j++) chunks += sg_chunks(jobs[j]);
    return align_up(4 * chunks, 256);
}

int sailor_hip_shadow_gather_instances_batched(SailorHipContext* ctx, const SailorPerInstanceData* dInstances, uint32_t numInstances,
                                               const SailorShadowGatherJob* jobs, uint32_t numJobs, void* dWorkspace, size_t workspaceBytes)
{
    if (!ctx || (numJobs != 0 && !jobs) || numInstances > 0x80000000u || ((uintptr_t)dInstances & 15)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    size_t chunks = 0;
    for (uint32_t j = 0; j < numJobs; j++) {
        const SailorShadowGatherJob& job = jobs[j];
        if (!job.dCount || ((uintptr_t)job.dCount & 3) || ((uintptr_t)job.dOut & 15) || ((uintptr_t)job.dMask & 7)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        if (job.begin > job.end || job.end > numInstances) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        if (job.end > job.begin && (!job.dMask || !dInstances || (job.capacity != 0 && !job.dOut))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        chunks += sg_chunks(job);
    }
    if (chunks != 0 && (!dWorkspace || ((uintptr_t)dWorkspace & 3))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (workspaceBytes < 4 * chunks) return SAILOR_HIP_ERR_WORKSPACE_TOO_SMALL;
    if (numJobs == 0) return SAILOR_HIP_OK;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* chunkOffset = (uint32_t*)dWorkspace;
    for (uint32_t j0 = 0; j0 < numJobs; j0 += SG_GROUP) {
        const uint32_t n = min(numJobs - j0, SG_GROUP);
        SgGroup g;
        memset(&g, 0, sizeof g);
        uint32_t total = 0;
        for (uint32_t j = 0; j < n; j++) {
            g.job[j] = jobs[j0 + j];
            g.chunkBase[j] = total;
            total += sg_chunks(jobs[j0 + j]);
        }
        for (uint32_t j = n; j <= SG_GROUP; j++) g.chunkBase[j] = total;
        sailor_launch(ctx, k_shadow_gather_scan, dim3(n), dim3(1024), g, chunkOffset);
        SAILOR_CHECK_LAUNCH(ctx, "k_shadow_gather_scan");
        if (total != 0) {
            sailor_launch(ctx, k_shadow_gather, dim3(total), dim3(SG_THREADS), (const float4*)dInstances, g, n, (const uint32_t*)chunkOffset);
            SAILOR_CHECK_LAUNCH(ctx, "k_shadow_gather");
        }
        chunkOffset += total;   // every group its own offsets
    }
    return SAILOR_HIP_OK;
}

int sailor_hip_shadow_gather_instances(SailorHipContext* ctx, const SailorPerInstanceData* dInstances, uint32_t numInstances, const uint64_t* dMask,
                                       uint32_t begin, uint32_t end, float* dOut, uint32_t capacity, uint32_t* dCount, void* dWorkspace, size_t workspaceBytes)
{
    SailorShadowGatherJob job;
    memset(&job, 0, sizeof job);
    job.dMask = dMask; job.begin = begin; job.end = end; job.dOut = dOut; job.capacity = capacity; job.dCount = dCount;
    return sailor_hip_shadow_gather_instances_batched(ctx, dInstances, numInstances, &job, 1, dWorkspace, workspaceBytes);
}

} // extern "C"
