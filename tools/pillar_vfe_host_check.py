#!/usr/bin/env python
"""csrc/pillar_vfe.hip compiled for the HOST and driven through the project's own Python route (crbhip/pillar_vfe.py, PillarVFE) on
host tensors: a check of the kernels' logic and of the binding that needs no GPU.

The kernels are compiled as plain C++ (same -ffp-contract=off) against a small stand-in for <hip/hip_runtime.h>: one std::thread per
GPU thread, the workgroups of a launch one after another, __shared__ as a static, __syncthreads as a pthread barrier. The lanes of a
wave do not run in lockstep here, so every exchange through LDS that leans on anything but a barrier shows up as a wrong result.
What this cannot show: memory behaviour, speed.
Checks (the cases and goldens of tests/pillar_cases.py): forward in train and eval mode against the f64 definition, backward and
running statistics against the torch route in f64, all in units of e_ref; garbage in the padded slots and a second call bit-equal.
Usage: python tools/pillar_vfe_host_check.py      (needs clang++, e.g. the one next to hipcc; CXX overrides)"""
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
// host emulation of the few HIP constructs csrc/pillar_vfe.hip uses: one std::thread per GPU thread, blocks one after another
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
extern thread_local dim3 threadIdx, blockIdx, blockDim;
extern pthread_barrier_t* g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(g_barrier); }
typedef void* hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
static inline hipError_t hipGetLastError() { return 0; }
static inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
static inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long c, unsigned long long v) {
  __atomic_compare_exchange_n(p, &c, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return c; }      // (crb_common.h's hash helpers)
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
template <typename T> static inline T __shfl_xor(T v, int, int) { return v; }
using std::min; using std::max;
template <typename K, typename... A>
static inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, A... args) {
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, block.x);
  g_barrier = &bar;
  for (unsigned b = 0; b < grid.x; ++b) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
      th.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(b); blockDim = block; kernel(args...); });
    for (auto& x : th) x.join();
  }
  pthread_barrier_destroy(&bar);
}
'''

HARNESS_CPP = r'''
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx, blockDim;
pthread_barrier_t* g_barrier;
#include "pillar_vfe.hip"
'''


def build(tmp):
    os.makedirs(os.path.join(tmp, 'hip'))
    open(os.path.join(tmp, 'hip', 'hip_runtime.h'), 'w').write(HIP_RUNTIME_H)
    open(os.path.join(tmp, 'harness.cpp'), 'w').write(HARNESS_CPP)
    csrc = os.path.join(ROOT, 'crb-active-3ddet_amd', 'csrc')
    cxx = os.environ.get('CXX') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    out = os.path.join(tmp, 'libpillar_vfe_host.so')
    subprocess.check_call([cxx, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-ffp-contract=off', '-w', '-I' + tmp, '-I' + csrc,
                           os.path.join(tmp, 'harness.cpp'), '-o', out, '-lpthread'])
    return ctypes.CDLL(out)


def install(H):
    """answer the pillar entry points of the C-ABI with the host build; let host tensors through to the fused route"""
    import crbhip
    from crbhip import pillar_vfe
    from pcdet.models.backbones_3d.vfe import pillar_vfe as mod
    for name, (ret, argtypes) in crbhip.parse_header().items():
        if 'pillar_vfe' in name:
            f = getattr(H, name)
            f.restype, f.argtypes = ret, argtypes

    class Lib:
        def __getattr__(self, k):
            return getattr(H, k) if 'pillar_vfe' in k else getattr(crbhip.lib, k)
    pillar_vfe.lib = Lib()
    pillar_vfe.require_cuda = lambda *a: None
    pillar_vfe.cur_stream = lambda d=None: None
    torch_forward = mod.PillarVFE.forward

    def forward(self, bd, **kw):
        v = bd['voxels']
        if v.dtype != torch.float32 or self.unsupported_reason(int(v.shape[2]), int(v.shape[1])) is not None:
            return torch_forward(self, bd, **kw)
        bd['pillar_features'] = self._forward_fused(v, bd['voxel_num_points'], bd['voxel_coords'])
        return bd
    mod.PillarVFE.forward = forward


def main():
    import pillar_cases as cases
    import test_pointpillar_cpu as cpu
    with tempfile.TemporaryDirectory() as tmp:
        install(build(tmp))
        gold = np.load(cases.GOLDEN)
        for name in cases.CASES:
            case = cases.make_case(name)
            C = case['voxels'].shape[2]
            w = cases.weights(C)
            for training in (True, False):
                tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
                res = cpu.run_vfe(cpu.make_vfe(C), case, name, training)
                ref = {'out': torch.from_numpy(cases.vfe_f64(case, w, training)['out'])}
                keys = ['out']
                if training:
                    ref.update({k: v for k, v in cpu.run_vfe(cpu.make_vfe(C, torch.float64), case, name, True, dtype=torch.float64).items() if k != 'out'})
                    keys += [k for k in cpu.TRAIN_KEYS if k != 'out']
                bad = cpu.check_against(res, ref, lambda k: gold['%s_e_ref_%s' % (tag, k)][0], keys, tag)
                assert not bad, bad
                again = cpu.run_vfe(cpu.make_vfe(C), case, name, training)
                assert all(torch.equal(res[k], again[k]) for k in res), 'second call differs'
        for training in (True, False):
            clean = cpu.run_vfe(cpu.make_vfe(4), cases.make_case('a'), 'a', training)
            for g in cases.GARBAGE:
                dirty = cpu.run_vfe(cpu.make_vfe(4), cases.make_case(g), 'a', training)
                assert all(torch.equal(clean[k], dirty[k]) for k in clean), g
        print('host build of csrc/pillar_vfe.hip: forward, backward and running statistics inside 4 x e_ref; garbage slots and a second '
              'call bit-equal')


if __name__ == '__main__':
    main()
