#!/usr/bin/env python
"""csrc/kitti_eval.hip compiled for the HOST and driven through the project's own Python route (crbhip/kitti_eval.py behind
get_official_eval_result(route='device')) on host tensors: a check of the kernels' logic and of the binding that needs no GPU, and
the way to find the cause of a wrong table.

The kernels are compiled as plain C++ (same -ffp-contract=off) against the HIP stand-in of tools/center_head_host_check.py: one
std::thread per GPU thread, the workgroups of a launch one after another, __shared__ as a static, __syncthreads as a pthread
barrier, atomicAdd as an __atomic builtin. The kernels use no wave intrinsics, so the very lines of the product are compiled: no
portable twin exists and no line differs. The lanes of a wave do not run in lockstep here, so an exchange through LDS that leans on
anything but a barrier shows up as a wrong result. What this cannot show: memory behaviour, speed, the f32 rounding of the GPU's
sinf / cosf / atan2f (the overlap bars below are the GPU test's, in the unit the golden records).
Checks (cases and bars of tests/test_kitti_eval_gpu.py): overlaps, true-positive scores, thresholds, counts, tables, result text
and dict of both golden cases, two runs bit-equal, the random size cases against the host route.
Usage: python tools/kitti_eval_host_check.py      (needs clang++, e.g. the one next to hipcc; CXX overrides)"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'crb-active-3ddet_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from center_head_host_check import HIP_RUNTIME_H  # noqa: E402

HARNESS_CPP = r'''
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
pthread_barrier_t* g_barrier;
#include "kitti_eval.hip"
'''


def build(tmp):
    os.makedirs(os.path.join(tmp, 'hip'))
    open(os.path.join(tmp, 'hip', 'hip_runtime.h'), 'w').write(HIP_RUNTIME_H)
    open(os.path.join(tmp, 'harness.cpp'), 'w').write(HARNESS_CPP)
    csrc = os.path.join(ROOT, 'crb-active-3ddet_amd', 'csrc')
    cxx = os.environ.get('CXX') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    out = os.path.join(tmp, 'libkitti_eval_host.so')
    subprocess.check_call([cxx, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-ffp-contract=off', '-w', '-I' + tmp, '-I' + csrc,
                           os.path.join(tmp, 'harness.cpp'), '-o', out, '-lpthread'])
    return ctypes.CDLL(out)


def install(H):
    """answer the crb_kitti_* entry points of the C-ABI with the host build; let host tensors through"""
    import crbhip
    from crbhip import kitti_eval
    for name, (ret, argtypes) in crbhip.parse_header().items():
        if 'crb_kitti' in name:
            f = getattr(H, name)
            f.restype, f.argtypes = ret, argtypes

    class Lib:
        def __getattr__(self, k):
            return getattr(H, k) if 'crb_kitti' in k else getattr(crbhip.lib, k)
    kitti_eval.lib = Lib()
    kitti_eval.DEVICE = 'cpu'


def main():
    import test_kitti_eval_gpu as gpu
    with tempfile.TemporaryDirectory() as tmp:
        install(build(tmp))
        for case in gpu.CASES:
            run = gpu.run_case(case)
            bad = gpu.check_case(case, run)
            assert not bad, bad
            assert gpu.same_bits(run, gpu.run_case(case)), case + ': second run differs'
        for name in gpu.SIZE_CASES:
            bad = gpu.check_sizes(name)
            assert not bad, bad
        print('host build of csrc/kitti_eval.hip: overlaps, true-positive scores, thresholds, counts, tables and result text of the '
              'golden cases inside the bars, a second run bit-equal; size cases equal to the host route')


if __name__ == '__main__':
    main()
