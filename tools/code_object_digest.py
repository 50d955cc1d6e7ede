#!/usr/bin/env python3
"""SHA-256 of the gfx950 code object's .text, .rodata, .note and .symtab sections, per translation unit.

"Bit-identical device code" made checkable without a GPU: run it on two trees (--root) and compare the output.  Every unit in
__graft_entry__.UNITS is compiled with the hipcc -c line of compile_library into a temporary directory, the code object is pulled out of
the object's .hip_fatbin, and the four sections are hashed.  (Two compiles of one source differ only in the __hip_cuid_* name in .dynstr,
which is why whole files are not compared; .symtab is hashed with its names resolved for the same reason: symbol_records.)  Nothing is
disassembled.

    python tools/code_object_digest.py [--root TREE] [hipcc flags, e.g. -DVSRD_CULL_INNER]
"""
import argparse
import hashlib
import importlib.util
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note", ".symtab")


def elf_sections(blob):
    """{name: bytes} of a little-endian ELF64 image."""
    assert blob[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    headers = [struct.unpack_from("<IIQQQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = blob[headers[shstrndx][4]:][:headers[shstrndx][5]]
    out = {}
    for name, kind, _flags, _addr, offset, size in headers:
        label = names[name:names.index(b"\0", name)].decode()
        out[label] = b"" if kind == 8 else blob[offset:offset + size]       # (8: SHT_NOBITS)
    return out


def symbol_records(sections):
    """.symtab with every st_name offset replaced by the name it points to and the per-compile suffix of __hip_cuid_<hash> dropped.
    That symbol's name is a hash of the source's path and text; the linker merges string tails in .strtab, so one other name moves the
    raw offsets of unrelated entries although no symbol, value, size or order has changed."""
    table, strings = sections[".symtab"], sections[".strtab"]
    out = []
    for at in range(0, len(table), 24):
        name, rest = struct.unpack_from("<I", table, at)[0], table[at + 4:at + 24]
        text = strings[name:strings.index(b"\0", name)]
        out.append(re.sub(rb"^__hip_cuid_[0-9a-f]+$", b"__hip_cuid_", text) + b"\0" + rest)
    return b"".join(out)


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--root", default=here, help="the tree to compile (default: the one this tool lives in)")
    args, extra_flags = parser.parse_known_args()
    root = os.path.abspath(args.root)
    spec = importlib.util.spec_from_file_location("_digest_entry", os.path.join(root, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)

    with tempfile.TemporaryDirectory() as tmp:
        units = list(entry.UNITS)
        for first in range(0, len(units), 2):                              # (at most two compiles side by side)
            batch = units[first:first + 2]
            running = [subprocess.Popen([entry.HIPCC, *entry.COMMON_FLAGS, *unit_flags, *extra_flags, "-c",
                                         os.path.join(entry.CSRC, name), "-o", os.path.join(tmp, name + ".o")], cwd=root)
                       for name, unit_flags in batch]
            if any([p.wait() for p in running]):
                sys.exit("hipcc -c failed")
        for name, _ in units:
            obj, fat, image = (os.path.join(tmp, name + ext) for ext in (".o", ".fatbin", ".co"))
            subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
            subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                            "--input=" + fat, "--output=" + image], check=True)
            with open(image, "rb") as f:
                sections = elf_sections(f.read())
            for section in SECTIONS:
                data = symbol_records(sections) if section == ".symtab" else sections[section]
                print(f"{name:<16} {section:<8} {len(data):>8}  {hashlib.sha256(data).hexdigest()}")


if __name__ == "__main__":
    main()
