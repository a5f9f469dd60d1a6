// kx_agent.h -- what a kernel body needs to hand data to ANOTHER launch that runs beside its own (the completion records of the
// level-3 parse, zstd_match.h, read by the entropy sweeps, zstd_entropy.h).  Requires kx_wave.h (the including translation unit
// provides it, as for zstd_common.h).  Compiled as HIP this is the product definition for gfx950; compiled as plain C++ (the CPU
// emulator of tests/emu, whose launches run one after the other in one memory) the stores are plain and the waits empty.
#pragma once

#if defined(__HIP__)
// A flag that workgroups of ANOTHER launch running beside this one read (the completion records of the level-3 parse, zstd_match.h):
// the L2s of the chiplets are not coherent by themselves.  The writer stores what the other launch reads, and the flag, with
// agent-scope stores, which go through its L2 to where every wave of the device reads them, and waits for them (kx_wait_stores)
// between the data and the flag: a release fence would do the same for plain stores, but it writes back the whole L2 -- 6.5 ms
// of a 185 ms parse at two fences a slice.  The reader's fence drops what its caches held from before the flag.
// kx_wait_stores / kx_fence_acquire_agent are called from wave-uniform control flow.
KX_DEV void kx_wait_stores() { __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); }     // every vector memory access of the wave so far has completed
KX_DEV void kx_fence_acquire_agent() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
KX_DEV void kx_st64_agent(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
KX_DEV void kx_st_agent(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
KX_DEV u32 kx_ld_agent(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
KX_DEV void kx_wait_stores() {}
KX_DEV void kx_fence_acquire_agent() {}
KX_DEV void kx_st64_agent(u64* p, u64 v) { *p = v; }
KX_DEV void kx_st_agent(u32* p, u32 v) { *p = v; }
KX_DEV u32 kx_ld_agent(const u32* p) { return *p; }
#endif
