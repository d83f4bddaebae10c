#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code in two builds of libgpubpe.so
(diagnostic, no GPU needed): a refactor of host code must leave every kernel's
instruction stream as it was.

    python tools/codeobj_diff.py parent/libgpubpe.so gpu-bpe_amd/lib/libgpubpe.so

Each library's .hip_fatbin section holds one offload bundle per translation
unit; every gfx950 code object in it is disassembled (llvm-objdump -d) and cut
at its function symbols.  Addresses, encodings and symbol annotations are
dropped, so only the instructions and their operands are compared (branches are
relative: moving a kernel does not change them).  Prints the functions that
exist on one side only, those whose instructions differ, and a summary line;
exit status 1 when anything differs.

    --rename 'REGEX=REPL'   applied to the second library's symbols before they are
                            matched (a kernel that gained a template argument)
    --notes REGEX           also print LDS bytes, scratch bytes, VGPRs, SGPRs and spills
                            (llvm-readelf --notes) of the second library's kernels whose
                            symbol matches
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    """the gfx950 code objects of every bundle in the library's .hip_fatbin"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib,
                    os.path.join(tmp, "unused")], check=True)
    blob = open(fat, "rb").read()
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n = int.from_bytes(blob[pos + 24:pos + 32], "little")
        q = pos + 32
        for _ in range(n):
            off, size, tlen = (int.from_bytes(blob[q + 8 * i:q + 8 * i + 8], "little") for i in range(3))
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + 1)
    return out


def functions(lib):
    """function symbol -> (instruction count, sha256 of its normalised instructions)"""
    fns = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib, tmp)):
            path = os.path.join(tmp, f"co{i}.o")
            open(path, "wb").write(co)
            asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path], check=True,
                                 capture_output=True, text=True).stdout
            name, body = None, []

            def close():
                if name is not None:
                    fns[name] = (len(body), hashlib.sha256("\n".join(body).encode()).hexdigest())

            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    close()
                    name, body = m.group(1), []
                elif name is not None and line.startswith("\t") and line.strip() != "...":   # ("...": elided zero padding)
                    ins = re.sub(r"//.*$", "", line)          # address (and encoding) comment
                    ins = re.sub(r"<[^>]*>", "", ins)         # symbol annotation of a branch target
                    body.append(" ".join(ins.split()))
            close()
    return fns


def notes(lib, pat):
    """resource usage of the kernels whose symbol matches pat, from the code objects' metadata notes"""
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib, tmp)):
            path = os.path.join(tmp, f"co{i}.o")
            open(path, "wb").write(co)
            out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], check=True, capture_output=True,
                                 text=True).stdout
            for blk in out.split("- .agpr_count")[1:]:
                f = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
                if re.search(pat, f("name")):
                    print(f"notes: {f('name')}: lds {f('group_segment_fixed_size')} scratch {f('private_segment_fixed_size')} "
                          f"vgpr {f('vgpr_count')} sgpr {f('sgpr_count')} vgpr spills {f('vgpr_spill_count')} "
                          f"sgpr spills {f('sgpr_spill_count')}")


def main():
    rename, pat = None, None
    while len(sys.argv) > 3 and sys.argv[1] in ("--rename", "--notes"):
        if sys.argv[1] == "--rename":
            rename = sys.argv[2].split("=", 1)
        else:
            pat = sys.argv[2]
        del sys.argv[1:3]
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    if rename:
        b = {re.sub(rename[0], rename[1], k): v for k, v in b.items()}
    if pat:
        notes(sys.argv[2], pat)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in only_a:
        print(f"only in {sys.argv[1]}: {k} ({a[k][0]} instructions)")
    for k in only_b:
        print(f"only in {sys.argv[2]}: {k} ({b[k][0]} instructions)")
    for k in differ:
        print(f"differs: {k} ({a[k][0]} -> {b[k][0]} instructions)")
    same = len(set(a) & set(b)) - len(differ)
    print(f"{len(a)} / {len(b)} device functions; {same} identical, {len(differ)} differ, "
          f"{len(only_a)} / {len(only_b)} on one side only; {sum(v[0] for v in b.values())} instructions compared")
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
