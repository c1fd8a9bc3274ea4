"""Build check of csrc/winograd_conv4.hip, csrc/winograd_wgrad4.hip and csrc/rows_gemm4.hip: the kernels name their accumulator AGPRs in inline asm, so the
compiler must not put anything of its own there. Compiles each file to ISA and fails if a compiler-generated v_accvgpr_write (VGPR
source) targets an accumulator register, or if a kernel uses scratch. The weight-gradient kernel also requests its pixels in inline
asm (global_load_dword, waited for by hand): between such a load and the counter wait that covers it nothing else may read or write
its destination register (the check follows the text of the loop, where every request is followed by its wait).
Usage: python tools/check_wino4_isa.py [--measure]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'crb-active-3ddet_amd', 'csrc')
SOURCES = (('winograd_conv4.hip', r'winograd4([bc]?)_kernel'), ('winograd_wgrad4.hip', r'winograd4_wgrad()_kernel'),
           ('rows_gemm4.hip', r'rows_gemm4()_(?:wgrad_)?kernel'))


def _regs(line):
    body = line.split(None, 1)[1] if ' ' in line else ''
    out = set()
    for a, b in re.findall(r'\bv\[(\d+):(\d+)\]', body):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r'\bv(\d+)\b', body))
    return out


def loads_in_flight(name, body):
    """asm loads of the main loop (between the first and the last MFMA of the kernel's text): destination untouched until a
    vmcnt wait with at most as many younger loads as it lets pass"""
    lines = [ln.strip() for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
    mf = [i for i, ln in enumerate(lines) if ln.startswith('v_mfma')]
    if not mf:
        return []
    lo, hi = mf[0], mf[-1]
    loads = [i for i in range(lo, hi) if lines[i].startswith('global_load_dword ')]
    bad = []
    for i in loads:
        d = int(re.match(r'global_load_dword v(\d+),', lines[i]).group(1))
        for j in range(i + 1, len(lines)):
            ln = lines[j]
            m = re.match(r's_waitcnt.*vmcnt\((\d+)\)', ln)
            if m and sum(1 for x in loads if i < x < j) >= int(m.group(1)):
                break
            if not ln.endswith(':') and d in _regs(ln):
                bad.append('%s: v%d of "%s" touched by "%s" before its wait' % (name, d, lines[i], ln))
                break
    return bad


def main(measure=False):
    bad = []
    for src, kern in SOURCES:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, 'w.s')
            cmd = ['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=off', '--cuda-device-only',
                   '-S', os.path.join(CSRC, src), '-o', out] + (['-DCRB_MEASURE'] if measure else [])
            subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
            text = open(out).read()
        found = 0
        for m in re.finditer(r'^(_ZN\S*' + kern + r'\S*):.*?s_endpgm', text, flags=re.S | re.M):
            name, body, second = m.group(1), m.group(0), m.group(2) == 'b'
            if 'wgrad_reduce' in name:
                continue
            found += 1
            if src == 'winograd_conv4.hip' and 'ILi9E' in name:           # the stamp build (mode 9) may clobber accumulators: timing only
                continue
            first_acc = 16 if second else 0
            for w in re.finditer(r'v_accvgpr_write_b32 a(\d+), v\d+', body):
                if int(w.group(1)) >= first_acc:
                    bad.append('%s: %s' % (name, w.group(0)))
            if re.search(r'\bscratch_(load|store)', body):
                bad.append('%s: scratch accesses' % name)
            if src == 'winograd_wgrad4.hip':
                bad += loads_in_flight(name, body)
        if not found:
            bad.append('%s: no kernel matched %s' % (src, kern))
    if bad:
        print('\n'.join(bad[:20]))
        raise SystemExit('the compiler touched registers the kernels manage by hand (%d findings)' % len(bad))
    print('winograd_conv4.hip / winograd_wgrad4.hip / rows_gemm4.hip ISA check ok (%s)' % ('measure' if measure else 'product'))


if __name__ == '__main__':
    main('--measure' in sys.argv)
