#!/usr/bin/env python3
"""Static table of every gfx950 kernel of a built library (needs no GPU): code size, VGPRs, SGPRs, scratch and static LDS.

    python tools/kernel_table.py upside-md_amd/csrc/libupside_hip.so [other.so]

The library's .hip_fatbin section holds one clang offload bundle per translation unit; each bundle's gfx950 code object is an ELF
whose NT_AMDGPU_METADATA note lists the kernels (llvm-readelf --notes) and whose symbol table gives the size of each kernel's code
(llvm-readelf --symbols).  With two libraries the tables are compared line by line (exit status 1 if they differ)."""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def code_objects(path):
    blob = open(path, 'rb').read()
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from('<Q', blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from('<QQQ', blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if 'gfx950' in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + 1)


def table(path):
    rows = []
    for elf in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(elf); f.flush()
            notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', f.name]).decode()
            syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--symbols', '--wide', f.name]).decode()
        size = {}
        for line in syms.splitlines():
            w = line.split()
            if len(w) == 8 and w[3] == 'FUNC':
                size[w[7]] = int(w[2], 0)
        for k in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            def field(name):
                return re.search(r'\.%s:\s+(\S+)' % name, k).group(1)
            name = field('name').strip("'")
            rows.append((name, size[name], int(field('vgpr_count')), int(field('sgpr_count')), int(field('private_segment_fixed_size')),
                         int(field('group_segment_fixed_size'))))
    if shutil.which('c++filt'):      # readable names where binutils is at hand
        plain = subprocess.check_output(['c++filt'], input='\n'.join(r[0] for r in rows).encode()).decode().splitlines()
        rows = [(re.sub(r'^void ', '', re.sub(r'\(.*', '', n)),) + r[1:] for n, r in zip(plain, rows)]
    rows.sort()
    return ['%7d %4d %4d %6d %6d  %s' % (r[1], r[2], r[3], r[4], r[5], r[0]) for r in rows]


def main():
    tabs = [table(p) for p in sys.argv[1:3]]
    head = '  bytes VGPR SGPR scratch   LDS  kernel'
    if len(tabs) == 1:
        print('\n'.join([head] + tabs[0]))
        return 0
    only_a = sorted(set(tabs[0]) - set(tabs[1])); only_b = sorted(set(tabs[1]) - set(tabs[0]))
    print('%s: %d kernels; %s: %d kernels' % (sys.argv[1], len(tabs[0]), sys.argv[2], len(tabs[1])))
    for tag, rows in (('<', only_a), ('>', only_b)):
        for r in rows:
            print(tag, r)
    print('tables identical' if tabs[0] == tabs[1] else 'tables differ')
    return 0 if tabs[0] == tabs[1] else 1


if __name__ == '__main__':
    sys.exit(main())
