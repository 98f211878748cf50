// The protocol of the layer-pipelined launches (gru_stack_generic_pipelined[_wrapped] in gru_kernels.hip, gru_stack_f16x3_pipelined
// in gru_f16x3_generic.hip): ONE grid of L x G workgroups, layer l consuming frame t of layer l - 1 as soon as it is published.
// Seams and counters live in FINE-GRAINED device memory (uncached in L2, coherent across XCDs), so no cache-wide acquire is needed
// -- an agent-scope acquire invalidates the L2 and with it the weight stream of every workgroup on the XCD, once per frame
// (measured: slower than the sequential launches).  A counter holds the number of frames of its group that are out.
#pragma once

namespace kws {

// cache-policy bits sc0 | sc1 of the seam's buffer loads and stores: system scope, past the non-coherent cache levels
constexpr int kSysScope = 1 | 16;

// blockIdx.x -> (layer, group); false: a padding block.  The inverse of pipelined_grid (launch.h): layer-major, or, XCD-affine
// (L divides 8; workgroups are dealt round-robin to the 8 XCDs), XCD x serves layer x % L only.  Either way a workgroup waits
// only for a block with a smaller index, and nobody waits for a padding block.
__device__ __forceinline__ bool pipelined_block(int L, int G, int xcd_affine, int& layer, int& group) {
    if (xcd_affine) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = 8 / L;
        layer = xcd % L;
        group = slot * per + xcd / L;
        if (group >= G) return false;           // grid padded to a multiple of 8
    } else {
        layer = blockIdx.x / G;
        group = blockIdx.x - layer * G;
    }
    return true;
}

// Consumer: frame t of the layer below must have landed (its workgroup runs concurrently on another CU).  Every wave polls for
// itself; the bound turns a protocol bug into a wrong answer plus an error flag instead of a hung GPU.
__device__ __forceinline__ void pipeline_wait(const int* ready_in, int* pipe_error, int group, int t, int lane) {
    int spins = 0;
    while (__hip_atomic_load(ready_in + group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= t) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1 << 24)) { if (lane == 0) *reinterpret_cast<volatile int*>(pipe_error) = 1; break; }
    }
    asm volatile("" ::: "memory");
}

// Producer, one thread: `frames` frames of the group are out.  Only behind a barrier that every wave reached with its seam stores
// drained (s_waitcnt vmcnt(0)) -- __syncthreads() itself does not wait for global stores, and a consumer on another CU must not
// see the counter before the rows (found by tools/stress_determinism.py).
__device__ __forceinline__ void pipeline_publish(int* ready_out, int group, int frames) {
    __hip_atomic_store(ready_out + group, frames, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Producer, whole workgroup, behind the frame loop: the last frame
__device__ __forceinline__ void pipeline_close(int* ready_out, int group, int T, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) pipeline_publish(ready_out, group, T);
}

}  // namespace kws
