#!/usr/bin/env python
"""csrc/center_head.hip compiled for the HOST and driven through the project's own Python route (crbhip/center_head.py) on host
tensors: a check of the kernels' logic and of the binding that needs no GPU, and the way to find the cause of a wrong result.

The kernels are compiled as plain C++ (same -ffp-contract=off) against a small stand-in for <hip/hip_runtime.h>: one std::thread per
GPU thread, the workgroups of a launch one after another over all three grid dimensions, __shared__ as a static, __syncthreads as a
pthread barrier, atomicMax / atomicAdd as __atomic_* builtins. The lanes of a wave do not run in lockstep here, so every exchange
through LDS that leans on anything but a barrier shows up as a wrong result. What this cannot show: memory behaviour, speed.
Checks (the cases and bars of tests/center_cases.py and tests/test_centerpoint_cpu.py): targets of every case against the golden,
with garbage rows, permuted overlaps and a second call bit-equal; losses forward and backward in NCHW and channels_last memory against
the reference's f64 values and the torch route in f64, two runs bit-equal; decoding in both layouts.
Usage: python tools/center_head_host_check.py      (needs clang++, e.g. the one next to hipcc; CXX overrides)"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'crb-active-3ddet_amd')):
    sys.path.insert(0, p)

HIP_RUNTIME_H = r'''
// host emulation of the few HIP constructs csrc/center_head.hip uses: one std::thread per GPU thread, blocks one after another
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <pthread.h>
#include <thread>
#include <vector>
#include <algorithm>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct int4 { int x, y, z, w; };
static inline int4 make_int4(int x, int y, int z, int w) { int4 r = {x, y, z, w}; return r; }
extern thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
extern pthread_barrier_t* g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(g_barrier); }
typedef void* hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
static inline hipError_t hipGetLastError() { return 0; }
static inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
static inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long c, unsigned long long v) {
  __atomic_compare_exchange_n(p, &c, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return c; }      // (crb_common.h's hash helpers)
static inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline int atomicMax(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return old; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
template <typename T> static inline T __shfl_xor(T v, int, int) { return v; }
using std::min; using std::max;
template <typename K, typename... A>
static inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, A... args) {
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, block.x);
  g_barrier = &bar;
  for (unsigned bz = 0; bz < grid.z; ++bz)
    for (unsigned by = 0; by < grid.y; ++by)
      for (unsigned bx = 0; bx < grid.x; ++bx) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; ++t)
          th.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(bx, by, bz); blockDim = block; gridDim = grid; kernel(args...); });
        for (auto& x : th) x.join();
      }
  pthread_barrier_destroy(&bar);
}
'''

HARNESS_CPP = r'''
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
pthread_barrier_t* g_barrier;
#include "center_head.hip"
'''


def build(tmp):
    os.makedirs(os.path.join(tmp, 'hip'))
    open(os.path.join(tmp, 'hip', 'hip_runtime.h'), 'w').write(HIP_RUNTIME_H)
    open(os.path.join(tmp, 'harness.cpp'), 'w').write(HARNESS_CPP)
    csrc = os.path.join(ROOT, 'crb-active-3ddet_amd', 'csrc')
    cxx = os.environ.get('CXX') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    out = os.path.join(tmp, 'libcenter_head_host.so')
    subprocess.check_call([cxx, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-ffp-contract=off', '-w', '-I' + tmp, '-I' + csrc,
                           os.path.join(tmp, 'harness.cpp'), '-o', out, '-lpthread'])
    return ctypes.CDLL(out)


def install(H):
    """answer the centre-head entry points of the C-ABI with the host build; let host tensors through to the fused route"""
    import crbhip
    from crbhip import center_head
    for name, (ret, argtypes) in crbhip.parse_header().items():
        if 'crb_center' in name:
            f = getattr(H, name)
            f.restype, f.argtypes = ret, argtypes

    class Lib:
        def __getattr__(self, k):
            return getattr(H, k) if 'crb_center' in k else getattr(crbhip.lib, k)
    center_head.lib = Lib()
    center_head.cur_stream = lambda d=None: None
    torch_route = center_head._why_torch
    center_head._why_torch = lambda *t: None if all(x is None or not x.is_floating_point() or x.dtype == torch.float32 for x in t) \
        else torch_route(*t)


def main():
    import warnings
    import center_cases as cases
    import test_centerpoint_cpu as cpu
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*torch route.*')
        install(build(tmp))
        for name in cases.TARGET_CASES:
            case, _ = cpu.targets_case(name)
            res = cpu.run_targets(case)
            bad = cpu.check_targets(res, name)
            assert not bad, bad
            for other in (cpu.run_targets(case), cpu.run_targets(case, gt=cases.garbage_rows(case['gt_boxes']))):
                assert all(np.array_equal(a[k], b[k]) for a, b in zip(res, other) for k in a), name + ': second call / garbage rows'
        case, _ = cpu.targets_case('edges')
        res, perm = cpu.run_targets(case), cpu.run_targets(case, gt=cases.permuted_overlaps(case['gt_boxes']))
        assert all(np.array_equal(a['heatmap'], b['heatmap']) for a, b in zip(res, perm)) and \
            not np.array_equal(res[0]['target_boxes'], perm[0]['target_boxes'])
        for name, h in cpu.LOSS_HEADS:
            case = cpu.loss_case(name, h)
            with cpu.quiet():
                ref64 = cpu.run_loss(case, dtype=torch.float64)
            for cl in (False, True):
                res = cpu.run_loss(case, channels_last=cl)
                bad = cpu.check_loss(res, ref64, name, h)
                assert not bad, bad
                again = cpu.run_loss(case, channels_last=cl)
                assert all(np.array_equal(res[k], again[k]) for k in res), 'second call differs'
        for name in cases.DECODE_CASES:
            for cl in (False, True):
                bad = cpu.check_decode(cpu.run_decode(cpu.decode_case(name), channels_last=cl), name)
                assert not bad, bad
        print('host build of csrc/center_head.hip: targets, losses (forward, backward; NCHW and channels_last) and decoding inside the '
              'bars; garbage rows, permuted overlaps and a second call bit-equal')


if __name__ == '__main__':
    main()
