#!/usr/bin/env python3
"""Which kernels does a build of csrc/ hold, and did a change leave the ones that remain alone?

    scripts/kernel_inventory.py <objdir>            per unit and per kernel template: instantiations,
                                                    bytes, byte-identical copies; totals
    scripts/kernel_inventory.py <objdir A> <objdir B>
                                                    kernel symbols of B that A lacks, symbols whose code
                                                    bytes or descriptor differ, symbols B removed;
                                                    exit status 1 on a new or a differing symbol

    make -C climatemachine.jl_amd/csrc OBJDIR=/tmp/a OUT=/tmp/a/libcmdg.so      (in each tree)

The gfx950 code object of every *.o is taken out of its .hip_fatbin section; every FUNC symbol of its
.dynsym is hashed over its own byte range, and the 64-byte kernel descriptor <symbol>.kd with bytes
16-23 masked: they hold the offset from the descriptor to the code, which moves when the layout of the
object moves.  Symbol tables and byte ranges only: nothing is looked for inside the code.  A kernel
instantiated in several units is compared against every copy of the same symbol in the other build.
scripts/compare_code_objects.sh compares whole units that must not change at all.
"""
import collections
import glob
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys

TARGET = b"hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


class Elf:
    """The little of a 64-bit little-endian ELF file that an inventory needs."""

    def __init__(self, data):
        assert data[:6] == b"\x7fELF\x02\x01", "not a 64-bit little-endian ELF file"
        self.data = data
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
        self.sections = []
        for i in range(shnum):
            name, typ, _flags, addr, off, size, link, _info, _align, entsize = struct.unpack_from(
                "<IIQQQQIIQQ", data, shoff + i * shentsize)
            self.sections.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link,
                                      entsize=entsize))
        strtab = self.sections[shstrndx]
        for s in self.sections:
            s["name"] = self._str(strtab, s["name"])

    def _str(self, strtab, at):
        start = strtab["off"] + at
        return self.data[start:self.data.index(b"\0", start)].decode()

    def section(self, name):
        return next((s for s in self.sections if s["name"] == name), None)

    def bytes_at(self, addr, size):
        for s in self.sections:
            if s["type"] != 8 and s["addr"] <= addr and addr + size <= s["addr"] + s["size"]:  # (8: NOBITS)
                start = s["off"] + addr - s["addr"]
                return self.data[start:start + size]
        raise ValueError("no section holds [%#x, +%d)" % (addr, size))

    def dynsyms(self):
        tab = self.section(".dynsym")
        if tab is None:
            return
        strtab = self.sections[tab["link"]]
        for i in range(tab["size"] // tab["entsize"]):
            name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", self.data,
                                                                        tab["off"] + i * tab["entsize"])
            yield self._str(strtab, name), info & 0xF, shndx, value, size


def code_object(path):
    """The gfx950 code object bundled in a host object, or None for a unit without device code."""
    host = Elf(open(path, "rb").read())
    fat = host.section(".hip_fatbin")
    if fat is None or fat["size"] == 0:
        return None
    blob = host.data[fat["off"]:fat["off"] + fat["size"]]
    if not blob.startswith(BUNDLE_MAGIC):
        raise ValueError("%s: .hip_fatbin is not an uncompressed offload bundle" % path)
    n, = struct.unpack_from("<Q", blob, len(BUNDLE_MAGIC))
    at = len(BUNDLE_MAGIC) + 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", blob, at)
        triple = blob[at + 24:at + 24 + tlen]
        at += 24 + tlen
        if triple == TARGET:
            return Elf(blob[off:off + size])
    return None


Kernel = collections.namedtuple("Kernel", "symbol size code kd")


def unit_kernels(path):
    """(bytes of .text, [Kernel]) of one object: every FUNC symbol with a descriptor."""
    co = code_object(path)
    if co is None:
        return 0, []
    syms = {name: (typ, value, size) for name, typ, shndx, value, size in co.dynsyms() if shndx != 0}
    out = []
    for name, (typ, value, size) in syms.items():
        if typ != 2 or name + ".kd" not in syms:  # (2: STT_FUNC)
            continue
        _t, kd_value, kd_size = syms[name + ".kd"]
        kd = bytearray(co.bytes_at(kd_value, kd_size))
        kd[16:24] = bytes(8)
        out.append(Kernel(name, size, hashlib.sha1(co.bytes_at(value, size)).hexdigest(),
                          hashlib.sha1(bytes(kd)).hexdigest()))
    text = co.section(".text")
    return (text["size"] if text else 0), out


def inventory(objdir):
    """{unit: (bytes of .text, [Kernel])} of the objects of a directory."""
    return {os.path.basename(o)[:-2]: unit_kernels(o) for o in sorted(glob.glob(os.path.join(objdir, "*.o")))}


def demangle(symbols):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return dict(zip(symbols, out.splitlines()))


def template_of(demangled):
    """'void cmdg::k_tendency<...>(...)' -> 'k_tendency'"""
    m = re.match(r"(?:void )?(?:\(anonymous namespace\)::|cmdg::)*([A-Za-z_][A-Za-z_0-9:]*)", demangled)
    return m.group(1) if m else demangled


def template_args(demangled):
    """The top-level template arguments of the kernel of a demangled symbol, as strings."""
    start = demangled.index("<")
    depth, args, cur = 0, [], ""
    for ch in demangled[start:]:
        if ch in "<(":
            depth += 1
            if depth == 1:
                continue
        elif ch in ">)":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    raise ValueError(demangled)


def by_template(kernels, names):
    groups = collections.defaultdict(list)
    for k in kernels:
        groups[template_of(names[k.symbol])].append(k)
    return groups


def report(objdir):
    inv = inventory(objdir)
    names = demangle(sorted({k.symbol for _t, ks in inv.values() for k in ks}))
    total = collections.defaultdict(lambda: [0, 0, 0])
    text_total = 0
    for unit, (text, kernels) in inv.items():
        if not kernels:
            continue
        text_total += text
        print("%s: .text %d bytes" % (unit, text))
        for tmpl, ks in sorted(by_template(kernels, names).items()):
            copies = len(ks) - len({k.code for k in ks})
            nbytes = sum(k.size for k in ks)
            print("  %-28s %4d instantiations %9d bytes %4d byte-identical copies" % (tmpl, len(ks), nbytes, copies))
            for i, v in enumerate((len(ks), nbytes, copies)):
                total[tmpl][i] += v
    print("all units: .text %d bytes" % text_total)
    for tmpl, (n, nbytes, copies) in sorted(total.items()):
        print("  %-28s %4d instantiations %9d bytes %4d byte-identical copies" % (tmpl, n, nbytes, copies))


def compare(dir_a, dir_b):
    def by_symbol(inv):
        d = collections.defaultdict(set)
        for unit, (_text, kernels) in inv.items():
            for k in kernels:
                d[k.symbol].add((k.code, k.kd))
        return d
    a, b = by_symbol(inventory(dir_a)), by_symbol(inventory(dir_b))
    names = demangle(sorted(set(a) | set(b)))
    new = sorted(s for s in b if s not in a)
    removed = sorted(s for s in a if s not in b)
    code_differs = sorted(s for s in b if s in a and not {c for c, _ in b[s]} <= {c for c, _ in a[s]})
    kd_differs = sorted(s for s in b if s in a and s not in code_differs and not b[s] <= a[s])
    for title, syms in (("new in " + dir_b, new), ("code bytes differ", code_differs),
                        ("descriptor differs outside bytes 16-23", kd_differs), ("removed in " + dir_b, removed)):
        print("%s: %d" % (title, len(syms)))
        for s in syms:
            print("  " + names[s])
    print("%d kernel symbols of %s are unchanged" % (len(b) - len(new) - len(code_differs) - len(kd_differs), dir_b))
    return 1 if new or code_differs or kd_differs else 0


if __name__ == "__main__":
    if len(sys.argv) == 2:
        report(sys.argv[1])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
