#!/usr/bin/env python3
"""device_code_diff.py REV [OBJECT ...]: is the gfx950 device code of the working tree that of REV?

Exports REV with `git archive`, takes every object's compile command from `make -n -B -C tnmf_amd/csrc` in both trees (so
the per-object flags come along), turns `-c X -o Y.o` into `--cuda-device-only -S X -o Y.s`, and compares the assembly as
text without the lines that name a __hip_cuid_ symbol (a hash of the translation unit).  Prints `identical` or the first
differing kernel symbol per object (OBJECT, e.g. `events fft_len_64`, restricts the list); exit status 1 on any difference.
Host only: needs hipcc, no GPU.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def commands(tree, out):
    """{object: (command that writes the device assembly of `tree`'s object to out/object.s, its directory)}"""
    csrc = os.path.join(tree, 'tnmf_amd', 'csrc')
    subprocess.run(['make', '-s', '-C', csrc, 'fft_len_twiddles.h'], check=True, stdout=subprocess.DEVNULL)
    dry = subprocess.run(['make', '-n', '-B', '-C', csrc], check=True, capture_output=True, text=True).stdout
    os.makedirs(out)
    found = (re.match(r'(\S*hipcc .*) -c (\S+) -o \S*/([^/\s]+)\.o$', line) for line in dry.splitlines())
    flags = '--cuda-device-only -Wno-unused-command-line-argument -S'
    return {m[3]: (f'{m[1]} {flags} {m[2]} -o {out}/{m[3]}.s', csrc) for m in found if m}


def first_difference(a, b):
    """None, or the last symbol defined before the first line in which the two files differ"""
    symbol = '(file head)'
    old, new = ([line for line in open(p) if '__hip_cuid_' not in line] for p in (a, b))
    for x, y in zip(old + [''], new + ['']):   # (the sentinel: one file a prefix of the other)
        if x != y:
            return symbol
        if re.match(r'[A-Za-z_][\w$.]*:', x):
            symbol = x.split(':')[0]
    return None if len(old) == len(new) else symbol


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'tree'))
        archive = subprocess.run(['git', '-C', ROOT, 'archive', sys.argv[1]], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', os.path.join(tmp, 'tree')], input=archive, check=True)
        old, new = commands(os.path.join(tmp, 'tree'), os.path.join(tmp, 'old')), commands(ROOT, os.path.join(tmp, 'new'))
        objects = sorted(o for o in old.keys() | new.keys() if o in sys.argv[2:] or not sys.argv[2:])
        jobs = [side[o] for side in (old, new) for o in objects if o in side]
        with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            for done in pool.map(lambda job: subprocess.run(job[0], shell=True, cwd=job[1]), jobs):
                done.check_returncode()
        where = {o: first_difference(f'{tmp}/old/{o}.s', f'{tmp}/new/{o}.s') if o in old and o in new else '(one tree only)'
                 for o in objects}
    for o in objects:
        print(f'{o:16s} identical' if where[o] is None else f'{o:16s} DIFFERS at {where[o]}')
    sys.exit(1 if any(w is not None for w in where.values()) else 0)


if __name__ == '__main__':
    main()
