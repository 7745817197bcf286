// lane_emu/hip/hip_runtime.h — TEST INFRASTRUCTURE, not product code: a stand-in for <hip/hip_runtime.h> that lets
// g++ compile the device headers (csrc/dev_math.h, id_eval.h, plant.h) unchanged for the host.  Put this directory in
// front of the include path; the headers then see the handful of HIP names they use, with these meanings:
//   __device__, __host__, __global__, __shared__, __launch_bounds__   nothing;  __forceinline__   inline
//   a lane                     one OS thread; a wavefront is up to 64 consecutive lanes, a block all of a launch's
//   threadIdx, blockIdx, blockDim   thread-locals, set by launch()
//   __shfl_xor                 a slot per lane of the wavefront, handed to the one lane that reads it by two counters.  It
//                              moves a register and is NO exchange point for LDS: under the thread sanitizer its atomics are
//                              relaxed, so that LDS accesses ordered by nothing but a butterfly are reported as a race
//   __builtin_amdgcn_wave_barrier   a pthread barrier over the wavefront's lanes
//   __syncthreads              a pthread barrier over the block's lanes
//   __builtin_amdgcn_fence     nothing (the barriers order the memory of OS threads)
// The block's dynamic LDS is the array idto_dev::lds, which the program defines; lds_prepare() fills the part a launch
// would request with NaN and poisons everything behind it for the address sanitizer.
//
// What a program built on this checks: the meaning of the C++ text on an abstract machine with sequentially consistent
// LDS whose lanes meet only at exchange points (wave_exchange_point) and barriers - indexing, association
// order, the LDS carve-up, initialisation (a read of LDS that nobody wrote yields NaN), a read or write beyond the dynamic
// LDS that the host asks for (a trap here; on the device a silent zero or a lost store), and, under the thread sanitizer,
// a missing exchange point or barrier (a data race here).
// What it cannot check: the device compiler's code generation, register allocation and spills, the lock-step execution
// of a real wavefront, the launch itself (its attributes, its arguments, the constant address space).
#pragma once

#include <pthread.h>

#include <sched.h>

#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <thread>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

#define __device__
#define __host__
#define __global__
#define __shared__
#define __forceinline__ inline
#define __launch_bounds__(...)

namespace lane_emu {

constexpr int kWave = 64;
struct Idx { int x, y, z; };
#if defined(__SANITIZE_THREAD__)
constexpr std::memory_order kPost = std::memory_order_relaxed, kSee = std::memory_order_relaxed;
#else
constexpr std::memory_order kPost = std::memory_order_release, kSee = std::memory_order_acquire;
#endif
struct Slot {
  std::atomic<double> value{0.0};
  std::atomic<unsigned> posted{0}, taken{0};   // shuffles this lane has posted a value for / whose value its reader has taken
};
struct Wave {
  pthread_barrier_t bar;
  int lanes;
  Slot slot[kWave];
};
struct Lane {
  Wave* wave = nullptr;
  pthread_barrier_t* block = nullptr;
  int lane = 0;
  unsigned shuffles = 0;
};
inline thread_local Lane self;

inline void wave_barrier() { pthread_barrier_wait(&self.wave->bar); }
inline void block_barrier() { pthread_barrier_wait(self.block); }
inline double shfl_xor(double x, int mask) {
  Wave* w = self.wave;
  const int from = self.lane ^ mask;
  if (from >= w->lanes) { std::fprintf(stderr, "lane_emu: __shfl_xor reads lane %d of a wavefront of %d\n", from, w->lanes); std::abort(); }
  // every shuffle has exactly one reader per slot (lane ^ mask is a bijection): post once the previous value is taken,
  // take the partner's once it is posted
  Slot& mine = w->slot[self.lane];
  Slot& theirs = w->slot[from];
  const unsigned n = self.shuffles++;
  while (mine.taken.load(kSee) != n) sched_yield();
  mine.value.store(x, kPost);
  mine.posted.store(n + 1, kPost);
  while (theirs.posted.load(kSee) != n + 1) sched_yield();
  const double r = theirs.value.load(kSee);
  theirs.taken.store(n + 1, kPost);
  return r;
}

// `usable` doubles of lds[total] are what the launch requests: NaN before every launch; the rest traps under ASan
inline void lds_prepare(double* lds, size_t total, size_t usable) {
  if (usable > total) { std::fprintf(stderr, "lane_emu: %zu doubles of LDS requested, the array has %zu\n", usable, total); std::abort(); }
  ASAN_UNPOISON_MEMORY_REGION(lds, total * sizeof(double));
  for (size_t i = 0; i < usable; ++i) lds[i] = std::numeric_limits<double>::quiet_NaN();
  ASAN_POISON_MEMORY_REGION(lds + usable, (total - usable) * sizeof(double));
}
inline void lds_release(double* lds, size_t total) { ASAN_UNPOISON_MEMORY_REGION(lds, total * sizeof(double)); }

}  // namespace lane_emu

inline thread_local lane_emu::Idx threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1};

namespace lane_emu {

// body() on `threads` lanes as block `block` of a launch; returns when every lane has
template <class F>
void launch(int block, int threads, F body) {
  const int nwaves = (threads + kWave - 1) / kWave;
  std::vector<Wave> waves(nwaves);
  pthread_barrier_t all;
  pthread_barrier_init(&all, nullptr, threads);
  for (int w = 0; w < nwaves; ++w) {
    waves[w].lanes = (w + 1 < nwaves) ? kWave : threads - w * kWave;
    pthread_barrier_init(&waves[w].bar, nullptr, waves[w].lanes);
  }
  std::vector<std::thread> pool;
  pool.reserve(threads);
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t]() {
      self.wave = &waves[t / kWave]; self.block = &all; self.lane = t % kWave; self.shuffles = 0;
      threadIdx = Idx{t, 0, 0}; blockIdx = Idx{block, 0, 0}; blockDim = Idx{threads, 1, 1};
      body();
    });
  for (std::thread& th : pool) th.join();
  for (int w = 0; w < nwaves; ++w) pthread_barrier_destroy(&waves[w].bar);
  pthread_barrier_destroy(&all);
}

}  // namespace lane_emu

#define __shfl_xor(x, mask) lane_emu::shfl_xor((x), (mask))
#define __syncthreads() lane_emu::block_barrier()
#define __builtin_amdgcn_wave_barrier() lane_emu::wave_barrier()
#define __builtin_amdgcn_fence(order, scope) ((void)0)
