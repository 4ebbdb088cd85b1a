#!/usr/bin/env python3
"""Per-kernel table of the gfx950 device code in the objects of a build directory, and the comparison of two builds in which
kernels may have moved between objects (a plain hash of an object's .text no longer compares then).

  tools/kernel_table.py DIR            one line per kernel: name | code hash, bytes | vgpr agpr sgpr scratch lds max_wg | object
  tools/kernel_table.py DIR_A DIR_B    what differs between the two builds, kernels matched by name

Code hash: sha256 of the bytes of the kernel's symbol in .text with the two things zeroed that depend on WHERE in a code object
the kernel lies, not on what it does: the literals of pc-relative address arithmetic (s_getpc_b64 followed by s_add_u32 /
s_addc_u32 with a literal: calls, constant tables), and the LDS kernel id (s_mov_b32 s15, <inline constant>: the index of the
kernel among those of its code object whose non-inlined callees find their LDS through the module's table; reported as `id`).
The comparison also covers the device functions that are not kernels (the callees of the generic-mode kernels)."""
import glob, hashlib, os, re, struct, subprocess, sys, tempfile
LLVM = '/opt/rocm/llvm/bin/'


def code_object_funcs(path):
    """{symbol: (hash, bytes, lds kernel ids seen)} of the FUNC symbols in .text of an AMDGPU code object"""
    b = open(path, 'rb').read()
    assert b[:4] == b'\x7fELF' and b[4] == 2
    shoff, = struct.unpack_from('<Q', b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', b, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from('<IIQQQQIIQQ', b, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    def cstr(tab, o):
        return b[tab['off'] + o:b.index(b'\0', tab['off'] + o)].decode()
    out = {}
    for s in secs:
        if s['type'] != 2:  # SHT_SYMTAB
            continue
        for k in range(s['size'] // s['entsize']):
            nm, info, _, shndx, value, size = struct.unpack_from('<IBBHQQ', b, s['off'] + k * s['entsize'])
            if (info & 0xf) != 2 or shndx == 0 or shndx >= len(secs) or cstr(secs[shstrndx], secs[shndx]['name']) != '.text':
                continue
            o = secs[shndx]['off'] + (value - secs[shndx]['addr'])
            w = list(struct.unpack_from('<%dI' % (size // 4), b, o))
            ids = set()
            for i in range(len(w)):
                if (w[i] & 0xFF80FFFF) == 0xBE801C00:  # s_getpc_b64
                    j = i + 1
                    while j < min(i + 8, len(w) - 1):
                        if (w[j] >> 24) in (0x80, 0x82) and 0xFF in (w[j] & 0xFF, (w[j] >> 8) & 0xFF):  # s_add(c)_u32 .., literal
                            w[j + 1] = 0
                            j += 2
                        else:
                            j += 1
                elif (w[i] & 0xFFFFFF00) == 0xBE8F0000 and 0x80 <= (w[i] & 0xFF) <= 0xC0:  # s_mov_b32 s15, 0..64
                    ids.add((w[i] & 0xFF) - 0x80)
                    w[i] &= 0xFFFFFF00
            out[cstr(secs[s['link']], nm)] = (hashlib.sha256(struct.pack('<%dI' % len(w), *w)).hexdigest()[:16], size, sorted(ids))
    return out


def kernel_meta(path):
    t = subprocess.run([LLVM + 'llvm-readelf', '--notes', path], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r'\n\s*- \.agpr_count', t)[1:]:
        blk = '.agpr_count' + blk
        g = lambda k: (re.search(r'\.' + k + r':\s*(\S+)', blk) or [None, '?'])[1]
        res[g('name')] = ' '.join(g(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size',
                                                   'group_segment_fixed_size', 'max_flat_workgroup_size'))
    return res


def table(d):
    """{symbol: (hash, bytes, ids, metadata or None for a device function that is no kernel, object)}"""
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(glob.glob(os.path.join(d, '*.o'))):
            base = os.path.basename(o)
            os.symlink(os.path.abspath(o), os.path.join(tmp, base))
            subprocess.run([LLVM + 'llvm-objdump', '--offloading', base], cwd=tmp, capture_output=True, check=True)
            for co in glob.glob(os.path.join(tmp, base) + '.*gfx950'):
                md = kernel_meta(co)
                for name, (h, size, ids) in code_object_funcs(co).items():
                    assert name not in rows or name not in md, name
                    rows[name if name in md else base + ':' + name] = (h, size, ids, md.get(name), base)
    return rows


def fmt(r):
    return f"{r[0]} {r[1]} B | {r[3]} | {r[4]}" + (f" id {','.join(map(str, r[2]))}" if r[2] else '')


if len(sys.argv) == 2:
    for name, r in sorted(table(sys.argv[1]).items()):
        if r[3]:
            print(f'{name} | {fmt(r)}')
else:
    A, B = table(sys.argv[1]), table(sys.argv[2])
    ka, kb = {k for k in A if A[k][3]}, {k for k in B if B[k][3]}
    print(f'# kernels: {len(ka)} | {len(kb)};  device functions that are no kernels: {len(A) - len(ka)} | {len(B) - len(kb)}')
    # a device function that is no kernel is keyed by object:name; match it by name alone where its object changed
    fa = {k.split(':', 1)[1]: v for k, v in A.items() if not v[3]}
    fb = {k.split(':', 1)[1]: v for k, v in B.items() if not v[3]}
    gone, new = sorted(ka - kb), sorted(kb - ka)
    differ = 0
    for k in sorted(ka & kb):
        a, b = A[k], B[k]
        if (a[0], a[1], a[3]) != (b[0], b[1], b[3]):
            differ += 1
            print(f'DIFFERS {k}\n    {fmt(a)}\n    {fmt(b)}')
    for k in sorted(set(fa) & set(fb)):
        if fa[k][:2] != fb[k][:2]:
            differ += 1
            print(f'DIFFERS (device function) {k}\n    {fmt(fa[k])}\n    {fmt(fb[k])}')
    print(f'# same-named kernels and device functions whose code or figures differ: {differ}')
    print(f'# device functions only in one build: {sorted(set(fa) ^ set(fb))}')
    print(f'# kernels only in the first build ({len(gone)}) / only in the second ({len(new)}), paired by code hash:')
    for k in gone:
        twins = [n for n in new if (B[n][0], B[n][1], B[n][3]) == (A[k][0], A[k][1], A[k][3])]
        print(f'  {k}  ->  {twins[0] if len(twins) == 1 else twins}   {fmt(A[k])}')
    for k in new:
        if not any((B[k][0], B[k][1], B[k][3]) == (A[g][0], A[g][1], A[g][3]) for g in gone):
            print(f'  (new) {k}   {fmt(B[k])}')
    print('# kernels in another object, or with another LDS kernel id:')
    for k in sorted(ka & kb):
        if A[k][4] != B[k][4] or A[k][2] != B[k][2]:
            print(f"  {k}: {A[k][4]}{' id ' + str(A[k][2]) if A[k][2] else ''} -> {B[k][4]}{' id ' + str(B[k][2]) if B[k][2] else ''}")
