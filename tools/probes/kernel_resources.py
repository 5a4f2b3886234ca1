"""What the compiler reports per kernel of a HIP source, without a GPU: registers, LDS, scratch and occupancy.

    python tools/probes/kernel_resources.py events.hip pursuit.hip [--root OTHER_CHECKOUT] [--no-lds KERNEL ...] [--only KERNEL ...]

Compiles tnmf_amd/csrc/<file> for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage and prints one
markdown row per kernel.  Exits 1 when a kernel uses scratch, when the device assembly holds a function call
(s_swappc_b64: something was not inlined), or when a kernel whose name starts with one of --no-lds has LDS -- the check
behind event_walk.h, whose Occurrence has to stay in registers:
    python tools/probes/kernel_resources.py events.hip pursuit.hip --no-lds k_events_update k_events_gain k_pursuit_pick
--only restricts the rows and the scratch check to kernels whose name starts with one of the given prefixes -- the row
behind fft.h's mix_rsh_waves() and mix_rsh_lds_bytes() (one line per atom height: VGPRs, LDS, no scratch):
    python tools/probes/kernel_resources.py fft_mixed.hip --only k_mix_reconstruct_sh
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FLAGS = ('-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-gpu-rdc -munsafe-fp-atomics '
         '-ffp-contract=fast --cuda-device-only -S -Rpass-analysis=kernel-resource-usage').split()
FIELDS = {'TotalSGPRs': 'SGPR', 'VGPRs': 'VGPR', 'LDS Size [bytes/block]': 'LDS', 'ScratchSize [bytes/lane]': 'scratch',
          'Occupancy [waves/SIMD]': 'occupancy'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sources', nargs='+')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--no-lds', nargs='*', default=[])
    ap.add_argument('--only', nargs='*', default=[])
    args = ap.parse_args()
    csrc = os.path.join(args.root, 'tnmf_amd', 'csrc')
    bad = []
    print('| kernel | ' + ' | '.join(FIELDS.values()) + ' |\n|---|' + '---|' * len(FIELDS))
    for name in args.sources:
        with tempfile.TemporaryDirectory() as tmp:
            asm = os.path.join(tmp, 'out.s')
            r = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS +
                               ['-I' + os.path.join(args.root, 'include'), '-I' + csrc, os.path.join(csrc, name), '-o', asm],
                               capture_output=True, text=True)
            if r.returncode:
                sys.exit(r.stderr)
            if 's_swappc_b64' in open(asm).read():
                bad.append(f'{name}: a function call in the device assembly')
        rows, kernel = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r'Function Name: (\S+)', line)
            if m:
                kernel = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip()
                kernel = re.sub(r'^(void )?\(anonymous namespace\)::', '', kernel).split('(')[0]
                rows[kernel] = {}
            m = re.search(r'remark.*:\s+(' + '|'.join(map(re.escape, FIELDS)) + r'): (\d+)', line)
            if m and kernel:
                rows[kernel][FIELDS[m.group(1)]] = int(m.group(2))
        for kernel, row in rows.items():
            if args.only and not any(kernel.startswith(k) for k in args.only):
                continue
            print(f'| `{kernel}` | ' + ' | '.join(str(row[f]) for f in FIELDS.values()) + ' |')
            if row['scratch']:
                bad.append(f'{kernel}: scratch')
            if row['LDS'] and any(kernel.startswith(k) for k in args.no_lds):
                bad.append(f'{kernel}: {row["LDS"]} bytes of LDS')
    for b in bad:
        print('FAILED', b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
