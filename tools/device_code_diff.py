#!/usr/bin/env python3
"""device_code_diff.py REV [OBJECT ...]: is the gfx950 device code of the working tree that of REV?

Exports REV with `git archive`, takes every object's compile command from `make -n -B -C tnmf_amd/csrc` in both trees (so
the per-object flags come along), turns `-c X -o Y.o` into `--cuda-device-only -S X -o Y.s`, and compares the assembly as
text without the lines that name a __hip_cuid_ symbol (a hash of the translation unit).  Prints `identical` per object
that matches as a whole (OBJECT, e.g. `events fft_len_64`, restricts the list).  An object that does not is compared kernel
by kernel: each kernel's text, with the function index taken out of its local labels (.LBB<index>_<n>: a kernel added or
removed in front of it renumbers them), and its entry in the .amdgpu_metadata block (register counts, LDS, private segment
and kernarg sizes); and what the object holds outside its kernels.  Printed are the kernels that are identical, changed,
only in REV and only in the working tree -- or that all of them are identical and only their order is not.  Exit status 1
on any changed kernel, a change outside the kernels, or an object that only one tree has.  Host only: needs hipcc, no GPU.
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


def assembly(path):
    return [line for line in open(path) if '__hip_cuid_' not in line]


def kernels(lines):
    """{kernel symbol: its text, function indices taken out, and its metadata entry}; under None: the rest of the file"""
    meta = next((i for i, line in enumerate(lines) if line.strip() == '.amdgpu_metadata'), len(lines))
    tail = next((i for i in range(meta) if lines[i].startswith('\t.section\t.AMDGPU.gpr_maximums')), meta)
    parts, name = {None: []}, None
    for line in lines[:tail]:
        begin = re.search(r'; -- Begin function (\S+)', line)
        if begin:   # (the line before it opens the function's section: .text, or one named after the function)
            previous, name = parts[name], begin[1]
            parts[name] = [previous.pop()] if previous and re.match(r'\t\.(text|section\t\.text)', previous[-1]) else []
        # (.LBB2_15 and .LBB12_15 become .LBB#_15; the comment behind a label starts at a fixed column where it can)
        parts[name].append(re.sub(r' +;', ' ;', re.sub(r'(\.L(?:BB|JTI|CPI|func_begin|func_end)|\bBB)\d+', r'\1#', line)))
    parts[None] += lines[tail:meta]
    for entry in re.split(r'^(?=  - \.)', ''.join(lines[meta:]), flags=re.M)[1:]:
        entry = re.split(r'^amdhsa\.', entry, flags=re.M)[0]   # (the last entry: what follows the list)
        parts[re.search(r'^    \.name: +(\S+)', entry, flags=re.M)[1]].append(entry)
    return {k: ''.join(v) for k, v in parts.items()}


def compare(a, b):
    """None where the two files are the same; else the kernel symbols (identical, changed, only in a, only in b), with None
    among the changed for a difference outside the kernels"""
    a, b = assembly(a), assembly(b)
    if a == b:
        return None
    old, new = kernels(a), kernels(b)
    return ([k for k in old if k and old[k] == new.get(k)], [k for k in old if k in new and old[k] != new[k]],
            [k for k in old if k not in new], [k for k in new if k not in old])


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'tree'))
        archive = subprocess.run(['git', '-C', ROOT, 'archive', rev], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', os.path.join(tmp, 'tree')], input=archive, check=True)
        old, new = commands(os.path.join(tmp, 'tree'), os.path.join(tmp, 'old')), commands(ROOT, os.path.join(tmp, 'new'))
        objects = sorted(o for o in old.keys() | new.keys() if o in sys.argv[2:] or not sys.argv[2:])
        jobs = [side[o] for side in (old, new) for o in objects if o in side]
        with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            for done in pool.map(lambda job: subprocess.run(job[0], shell=True, cwd=job[1]), jobs):
                done.check_returncode()
        found = {o: compare(f'{tmp}/old/{o}.s', f'{tmp}/new/{o}.s') if o in old and o in new else 'DIFFERS: in one tree only'
                 for o in objects}
    failed = False
    for o in objects:
        if found[o] is None or isinstance(found[o], str):
            print(f'{o:16s} {found[o] or "identical"}')
            failed |= found[o] is not None
            continue
        lists = dict(zip(('identical', 'CHANGED', f'only in {rev}', 'only in the working tree'), found[o]))
        if not any(v for k, v in lists.items() if k != 'identical'):
            print(f'{o:16s} identical kernel by kernel ({len(found[o][0])}) and outside the kernels; their order differs')
            continue
        print(f'{o:16s} DIFFERS as a whole; kernel by kernel: ' + ', '.join(f'{len(v)} {k}' for k, v in lists.items()))
        for title, names in lists.items():
            for k in names:
                print(f'    {title + ":":26s}{k or "(outside the kernels)"}')
        failed |= bool(lists['CHANGED'])
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
