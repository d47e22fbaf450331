// Cold-operand prefetch shared by the kernels that host it (gemm_dual.hip, layer_norm.hip): the first ``pf.wgs``
// workgroups of a launch read up to two byte ranges once, one 4-B load per 64-B granule, so the ranges are
// cache-resident (Infinity Cache) when the kernels that follow touch them.  They run beside the launch's own work,
// which leaves HBM bandwidth unused.  Loads only: nothing is written.
#pragma once

struct Prefetch {
  const char* p[2];
  long bytes[2];
  int wgs;
};

__device__ __forceinline__ void prefetch_part(const Prefetch& pf, int part) {
  unsigned acc = 0u;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (!pf.p[r] || pf.bytes[r] <= 0) continue;
    const long gran = (pf.bytes[r] + 63) / 64;
    const long per = (gran + pf.wgs - 1) / pf.wgs;
    const long g0 = (long)part * per;
    const long g1 = g0 + per < gran ? g0 + per : gran;
    const char* base = pf.p[r];
    for (long g = g0 + threadIdx.x; g < g1; g += (long)blockDim.x * 8) {
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long gg = g + (long)u * blockDim.x;
        v[u] = gg < g1 ? *(const unsigned*)(base + gg * 64) : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc ^= v[u];
    }
  }
  asm volatile("" ::"v"(acc));  // keep the loads
}
