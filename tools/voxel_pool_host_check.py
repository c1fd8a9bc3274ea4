#!/usr/bin/env python
"""csrc/voxel_pool.hip compiled for the HOST and driven through the project's own Python route (crbhip/voxel_pool.py,
NeighborVoxelSAModuleMSG, VoxelRCNNHead) on host tensors: a check of the kernels' logic and of the binding that needs no GPU.

The kernels are compiled as plain C++ (same -ffp-contract=off) against a small stand-in for <hip/hip_runtime.h>: one std::thread per
GPU thread, the workgroups of a launch one after another, __shared__ as a static, __syncthreads as a pthread barrier, atomics as
compare-and-swap loops. What this cannot show: the device's atomic ordering, memory behaviour, speed.
Checks (the cases and goldens of tests/voxel_rcnn_cases.py): query indices equal the restatement; the fused pooling against the f64
definition in units of e_ref; whole-module steps (train and eval mode) against the golden and against the torch route in f64; the
head's eval pass and training step against the golden; two head steps under deterministic algorithms bit-identical.
Usage: python tools/voxel_pool_host_check.py      (needs clang++, e.g. the one next to hipcc; CXX overrides)"""
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
// host emulation of the few HIP constructs csrc/voxel_pool.hip uses: one std::thread per GPU thread, blocks one after another
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
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct int4 { int x, y, z, w; };
static inline int4 make_int4(int a, int b, int c, int d) { return int4{a, b, c, d}; }
extern thread_local dim3 threadIdx, blockIdx, blockDim;
extern pthread_barrier_t* g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(g_barrier); }
typedef void* hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
static inline hipError_t hipGetLastError() { return 0; }
static inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
template <typename T> static inline T __shfl_xor(T v, int, int) { return v; }
using std::min; using std::max;
static inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long c, unsigned long long v) {
  __atomic_compare_exchange_n(p, &c, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return c; }
static inline float atomicAdd(float* p, float v) {
  float o = *p, n;
  do { n = o + v; } while (!__atomic_compare_exchange(p, &o, &n, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST));
  return o; }
static inline int atomicMin(int* p, int v) { int o = *p; while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} return o; }
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
#include "voxel_pool.hip"
extern "C" void host_hash_build(const int* coords, int n, int D, int H, int W, long long* hkeys, int* hvals, long long cap) {
  memset(hkeys, 0xff, cap * 8); memset(hvals, 0x7f, cap * 4);
  for (int i = 0; i < n; ++i) {
    const int* c = coords + 4 * i;
    long long key = (((long long)c[0] * D + c[1]) * H + c[2]) * (long long)W + c[3];
    uint32_t slot = crb_ghash_insert(hkeys, (uint32_t)(cap - 1), key);
    if (hvals[slot] > i) hvals[slot] = i;
  }
}
extern "C" long long host_hash_cap(long long n) { return crb_hash_capacity(n); }
'''

NAMED = ('grad/features', 'grad/mlps_pos.0.0.weight', 'grad/mlps_pos.0.1.weight', 'grad/mlps_pos.0.1.bias',
         'buf/mlps_pos.0.1.running_mean', 'buf/mlps_pos.0.1.running_var')


def build(tmp):
    os.makedirs(os.path.join(tmp, 'hip'))
    open(os.path.join(tmp, 'hip', 'hip_runtime.h'), 'w').write(HIP_RUNTIME_H)
    open(os.path.join(tmp, 'harness.cpp'), 'w').write(HARNESS_CPP)
    csrc = os.path.join(ROOT, 'crb-active-3ddet_amd', 'csrc')
    cxx = os.environ.get('CXX') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    out = os.path.join(tmp, 'libvoxel_pool_host.so')
    subprocess.check_call([cxx, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-ffp-contract=off', '-w', '-I' + tmp, '-I' + csrc,
                           os.path.join(tmp, 'harness.cpp'), '-o', out, '-lpthread'])
    return ctypes.CDLL(out)


def install(H):
    """answer the voxel entry points of the C-ABI and the site hash with the host build; let host tensors through"""
    import crbhip
    from crbhip import sparse, voxel_pool
    from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as vpm
    H.host_hash_cap.restype, H.host_hash_cap.argtypes = ctypes.c_longlong, [ctypes.c_longlong]
    for name, (ret, argtypes) in crbhip.parse_header().items():
        if 'voxel_pool' in name or 'voxel_query' in name:
            f = getattr(H, name)
            f.restype, f.argtypes = ret, argtypes

    class Lib:
        def __getattr__(self, k):
            return getattr(H, k) if ('voxel_pool' in k or 'voxel_query' in k) else getattr(crbhip.lib, k)
    voxel_pool.lib = Lib()
    voxel_pool.require_cuda = lambda *a: None
    voxel_pool.cur_stream = lambda d=None: None

    def build_hash(coords, shape):
        n = coords.shape[0]
        cap = H.host_hash_cap(n)
        hk, hv = torch.empty(cap, dtype=torch.int64), torch.empty(cap, dtype=torch.int32)
        H.host_hash_build(ctypes.c_void_p(coords.data_ptr()), ctypes.c_int(n), ctypes.c_int(shape[0]), ctypes.c_int(shape[1]),
                          ctypes.c_int(shape[2]), ctypes.c_void_p(hk.data_ptr()), ctypes.c_void_p(hv.data_ptr()), ctypes.c_longlong(cap))
        return hk, hv, cap
    sparse.build_hash = build_hash

    def fused_route(self, k, f, sp):              # the module's own rule without its "device tensors only" clause
        if not vpm.voxel_query_utils._is_sparse_tensor(sp):
            return 'dense'
        if self.pool_method == 'avg_pool' and torch.are_deterministic_algorithms_enabled() and f.requires_grad:
            return 'avg_pool under deterministic algorithms'
        return None
    vpm.NeighborVoxelSAModuleMSG.fused_route = fused_route


def main():
    import voxel_rcnn_cases as cases
    import test_voxel_rcnn_cpu as cpu
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import _rows
    with tempfile.TemporaryDirectory() as tmp:
        install(build(tmp))
        gold = np.load(cases.GOLDEN)
        for name in cases.LEVEL_CASES:
            p = cases.level_case(name)
            q = cases.case_query_inputs(p)
            for pool in cases.POOLS:
                for training in (True, False):
                    tag = 'm_%s_%s_%s' % (name, pool, 'train' if training else 'eval')
                    kw = cpu.module_inputs(p, q, sparse=True)
                    mod = cpu.make_module(p, pool).train(training)
                    ref_mod = cpu.make_module(p, pool)
                    bn = ref_mod.mlps_pos[0][1]
                    with torch.no_grad():
                        fin = _rows(mod.mlps_in[0], kw['features'])
                        new_coords = torch.from_numpy(q[2])
                        pooled = mod._pool_fused(0, fin, kw['xyz'], kw['new_xyz'], new_coords, kw['voxel2point_indices'])
                    from pcdet.ops.pointnet2.pointnet2_stack import voxel_query_utils
                    idx, cnt = voxel_query_utils.voxel_query_hip(p['ranges'], p['radius'], p['nsample'], kw['xyz'], kw['new_xyz'], new_coords,
                                                                 kw['voxel2point_indices'])
                    assert np.array_equal(idx.numpy(), gold['q_%s_idx' % name]) and np.array_equal((cnt == 0).numpy(), gold['q_%s_empty' % name])
                    stats = {} if training else {'mean': bn.running_mean.numpy(), 'var': bn.running_var.numpy()}
                    f64 = cases.pool_f64(fin.numpy(), q[0], q[1], gold['q_%s_idx' % name], gold['q_%s_empty' % name],
                                         ref_mod.mlps_pos[0][0].weight.detach().numpy(), bn.weight.detach().numpy(), bn.bias.detach().numpy(),
                                         bn.eps, pool, **stats)[0]
                    r_pool = float(np.abs(pooled.numpy() - f64).max()) / float(gold[tag + '_pooled_e_ref'][0])
                    res = cpu.run_module(cpu.make_module(p, pool), p, cpu.module_inputs(p, q, sparse=True), training)
                    cpu.assert_matches_golden(gold, tag, res)
                    r64 = cpu.run_module(cpu.make_module(p, pool).double(), p, cpu.module_inputs(p, q, dtype=torch.float64), training)
                    rs = {k: float((res[k].double() - r64[k]).abs().max()) / float(gold['%s_e_ref_%s' % (tag, k)][0])
                          for k in r64 if r64[k].dtype.is_floating_point}
                    print('%-22s query exact; pooling %.2f x e_ref; step vs torch route f64: named %.2f, all %.2f x e_ref' % (
                        tag, r_pool, max(v for k, v in rs.items() if k in NAMED), max(rs.values())))
        cpu.check_head_train_step(gold, cpu.head_train_step())
        for tag, dp in (('dp0', 0.0), ('dp3', 0.3)):
            with torch.no_grad():
                bd = cpu.make_head(dp).eval()(cpu.head_batch())
            np.testing.assert_allclose(bd['batch_cls_preds'].numpy(), gold['head_eval_cls_' + tag], rtol=1e-4, atol=1e-5)
        runs = []
        torch.use_deterministic_algorithms(True)
        try:
            for _ in range(2):
                head = cpu.head_train_step()
                loss, _ = head.get_loss()
                head.zero_grad()
                loss.backward()
                runs.append((loss.detach().clone(), {n: t.grad.clone() for n, t in head.named_parameters()}))
        finally:
            torch.use_deterministic_algorithms(False)
        assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][n], runs[1][1][n]) for n in runs[0][1])
        print('head: eval pass and training step match the golden; two deterministic steps are bit-identical')


if __name__ == '__main__':
    main()
