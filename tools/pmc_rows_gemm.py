#!/usr/bin/env python
"""Minimal driver for counter passes over the split-bf16 row-GEMM forward kernel (csrc/rows_gemm4.hip): three launches of each of the two
bench layers (16 x 256 -> 256 k2s2 @ 100 x 88, 16 x 128 -> 256 k1s1 @ 200 x 176), nothing else on the device.
  rocprofv3 --pmc FETCH_SIZE --kernel-include-regex rows_gemm4_kernel --output-format csv -d DIR -o p -- python tools/pmc_rows_gemm.py
(counters only, one counter per pass; FETCH_SIZE / WRITE_SIZE are in KiB). tools/pmc_rows_gemm.py --sum DIR... prints the average per
launch of every counter file under the directories, in launch order (k2s2 first)."""
import csv
import glob
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))


def summarise(dirs):
    for d in dirs:
        for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
            rows = [r for r in csv.DictReader(open(f)) if 'rows_gemm4_kernel' in r['Kernel_Name']]
            rows.sort(key=lambda r: int(r['Dispatch_Id']))
            for name in sorted({r['Counter_Name'] for r in rows}):
                vals = [float(r['Counter_Value']) for r in rows if r['Counter_Name'] == name]
                half = len(vals) // 2
                for label, v in (('k2s2 forward (algorithmic 0.72 GB)', vals[:half]), ('k1s1 forward (algorithmic 0.87 GB)', vals[half:])):
                    if v:
                        print('%-12s %-36s %10.1f KiB per launch = %.3f GB (%d launches)'
                              % (name, label, sum(v) / len(v), sum(v) / len(v) * 1024 / 1e9, len(v)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--sum':
        summarise(sys.argv[2:])
        sys.exit(0)
    import torch
    from crbhip import rows_gemm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    for cin, cout, s, H, W in ((256, 256, 2, 100, 88), (128, 256, 1, 200, 176)):
        x = torch.randn(16, cin, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        w = torch.randn(cin, cout, s, s, device=dev) / cin ** 0.5
        for _ in range(3):
            rows_gemm.forward_x6(x, w, cin, cout, s)
        torch.cuda.synchronize()
    print('PMC_ROWS_GEMM done')
