// Does a flag word that one wave stores after a group of LDS stores, with no
// wait between, become visible only after those stores?  (The match kernel's
// link waves publish their progress that way: csrc/deflate.hip,
// chain_link_groups.)  One workgroup of 16 waves.  Wave 0 writes round number
// r into K words -- eight stores per lane, u32 and u16 in turn, to scattered
// banks -- and then r into the flag (lane 0), R rounds without any wait.
// Waves 1-7 poll the flag with an acquire load, then read the K words and
// count the words older than the flag they saw.  Waves 8-15 keep the LDS busy
// with random reads.  Every loop is bounded: a reader gives up after a fixed
// number of polls and reports it.  Prints the stale-word count over all
// launches; exit status 1 on a stale word, a give-up or no flag seen in flight.
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr int K = 512;          // words the writer fills per round (8 per lane)
constexpr int R = 1500;         // rounds per launch (< 2^16: the u16 stores hold r)
constexpr int NOISE = 8192;     // words the noise waves read
constexpr int MAX_POLLS = 1 << 18;

struct Shared {
  unsigned w[K];
  unsigned flag;
  unsigned pad[15];
  unsigned noise[NOISE];
};

__device__ __forceinline__ unsigned lds_addr(const void *p) { return (unsigned)(size_t)p; }
// a read the compiler keeps and issues as an LDS instruction (a volatile access through a cast would go out as a flat load)
__device__ __forceinline__ unsigned lds_read(unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// out[0]: stale words, [1]: give-ups, [2]: flag values seen while the writer was still running, [3]: sink
__global__ __launch_bounds__(1024) void k(unsigned *out, int pause) {
  __shared__ Shared s;
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (unsigned i = t; i < K; i += 1024) s.w[i] = 0;
  for (unsigned i = t; i < NOISE; i += 1024) s.noise[i] = i * 2654435761u;
  if (t == 0) s.flag = 0;
  __syncthreads();
  if (wave == 0) {
    unsigned a[8];
    for (int j = 0; j < 8; ++j) a[j] = lds_addr(&s.w[((j * 64 + lane) * 37u) & (K - 1)]);  // (37 odd: a permutation)
    const unsigned fa = lds_addr(&s.flag);
    for (unsigned r = 1; r <= (unsigned)R; ++r) {
      asm volatile(
          "ds_write_b32 %0, %8\n\tds_write_b16 %1, %8\n\tds_write_b32 %2, %8\n\tds_write_b16 %3, %8\n\t"
          "ds_write_b32 %4, %8\n\tds_write_b16 %5, %8\n\tds_write_b32 %6, %8\n\tds_write_b16 %7, %8" ::"v"(a[0]),
          "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(r)
          : "memory");
      if (lane == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(fa), "v"(r) : "memory");
      if (pause) __builtin_amdgcn_s_sleep(2);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  } else if (wave < 8) {
    unsigned stale = 0, seen = 0, last = 0, gave_up = 0;
    for (int polls = 0;;) {
      const unsigned f = (unsigned)__builtin_amdgcn_readfirstlane(
          (int)__hip_atomic_load(&s.flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (f != last) {
        for (int j = 0; j < 8; ++j) {
          const unsigned v = lds_read(&s.w[(j * 64 + lane + wave * 8) & (K - 1)]);
          stale += v < f;
        }
        seen += (lane == 0 && f < (unsigned)R);
        last = f;
      }
      if (f >= (unsigned)R) break;
      if (++polls >= MAX_POLLS) {
        gave_up = lane == 0;
        break;
      }
    }
    if (stale) atomicAdd(&out[0], stale);
    if (gave_up) atomicAdd(&out[1], 1u);
    if (seen) atomicAdd(&out[2], seen);
  } else {
    unsigned x = t * 2246822519u + 1u, acc = 0;
    for (int i = 0; i < 20000; ++i) {
      x = x * 1664525u + 1013904223u;
      acc += lds_read(&s.noise[(x >> 8) & (NOISE - 1)]);
      if ((i & 63) == 63 &&
          (unsigned)__builtin_amdgcn_readfirstlane((int)lds_read(&s.flag)) >= (unsigned)R)
        break;
    }
    if (acc == 0x12345u) out[3] = acc;
  }
}

int main() {
  unsigned *d, h[4];
  if (hipMalloc(&d, 16) != hipSuccess) return 2;
  unsigned long long stale = 0, gave_up = 0, seen = 0;
  const int launches = 400;
  for (int rep = 0; rep < launches; ++rep) {
    if (hipMemset(d, 0, 16) != hipSuccess) return 2;
    hipLaunchKernelGGL(k, dim3(1), dim3(1024), 0, 0, d, rep & 1);
    if (hipMemcpy(h, d, 16, hipMemcpyDeviceToHost) != hipSuccess) {
      printf("launch %d failed: %s\n", rep, hipGetErrorString(hipGetLastError()));
      return 2;
    }
    stale += h[0];
    gave_up += h[1];
    seen += h[2];
  }
  const bool ok = stale == 0 && gave_up == 0 && seen > 0;
  printf("flag after stores: %s (%llu stale words, %llu give-ups, %llu flag values read in flight, %d launches)\n",
         ok ? "yes" : "NO", stale, gave_up, seen, launches);
  return ok ? 0 : 1;
}
