"""Are the device kernels of two builds of the library the same?  Symbol by symbol, so host code may move between translation units.
  python profiles/tools/isa_diff.py <a/libsdxlstep.so> <b/libsdxlstep.so> [...more pairs]
Every gfx950 code object is cut out of the library's offload bundles, disassembled (llvm-objdump -d) and split by function symbol; the
kernels' metadata notes (registers, LDS, scratch, workgroup size, arguments) are compared too.  Exit status 1 if anything differs."""
import re, struct, subprocess, sys, tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so):
    blob = Path(so).read_bytes()
    at = -1
    while (at := blob.find(MAGIC, at + 1)) >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        q = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]


def symbols(so):
    """{function symbol: disassembly}, {kernel: metadata}"""
    funcs, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(so)):
            f = Path(tmp) / f"{i}.co"
            f.write_bytes(co)
            dis = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", f], capture_output=True, text=True, check=True).stdout
            syms = sorted((int(m[0], 16), int(m[1]), m[2]) for m in re.findall(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(?:OBJECT|FUNC)\s+\S+\s+\S+\s+\d+\s+(\S+)$",
                          subprocess.run([LLVM / "llvm-readelf", "-sW", f], capture_output=True, text=True, check=True).stdout, re.M))

            def where(addr):      # an address as symbol + offset
                hit = [s for s in syms if s[0] <= addr < s[0] + max(s[1], 1)]
                return f"<{hit[0][2]}+{addr - hit[0][0]:#x}>" if hit else f"<unknown {addr:#x}>"
            for name, body in re.findall(r"^<([^>\n]+)>:\n(.*?)(?=^<[^>\n]+>:\n|\Z)", dis, re.S | re.M):
                assert name not in funcs, name
                # pc-relative addresses (s_getpc_b64 sN, then s_add_u32 sN, sN, literal) are named by what they point at, and the trailing comment
                # (address, encoding) goes: the kernels may sit elsewhere in the code object
                out, pc = [], {}
                for line in body.splitlines():
                    text, _, note = line.partition("//")
                    text = text.strip()
                    if m := re.match(r"s_getpc_b64 s\[(\d+):", text):
                        pc[m[1]] = int(note.split(":")[0], 16) + 4
                    elif (m := re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+)$", text)) and m[1] == m[2] and m[1] in pc:
                        lit = int(m[3], 16)
                        text = f"s_add_u32 s{m[1]}, s{m[1]}, {where(pc.pop(m[1]) + (lit - (1 << 32) if lit >> 31 else lit))}"
                    if text != "...":      # (objdump's mark for the zero padding up to the next symbol)
                        out.append(text)
                while out and out[-1] in ("s_nop 0", ""):      # (the filler behind the function's last instruction: its length depends on what follows
                    out.pop()                            # the function in its code object -- the last one of a translation unit gets a long run)
                funcs[name] = "\n".join(out).strip()
            notes = subprocess.run([LLVM / "llvm-readelf", "--notes", f], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"^\s*- (?=\.agpr_count:|\.args:)", notes, flags=re.M)[1:]:
                m = re.search(r"^\s*\.name:\s*(\S+)", blk, re.M)
                if m:
                    blk = blk.split("amdhsa.target:")[0].split("amdhsa.version:")[0]
                    meta[m.group(1)] = "\n".join(l.strip() for l in blk.splitlines() if l.strip())
    return funcs, meta


bad = 0
for a, b in zip(sys.argv[1::2], sys.argv[2::2]):
    (fa, ma), (fb, mb) = symbols(a), symbols(b)
    assert ma and set(ma) <= set(fa), "no kernels found"
    only = sorted(set(ma) ^ set(mb))
    isa = sorted(k for k in set(ma) & set(mb) if fa[k] != fb[k])
    md = sorted(k for k in set(ma) & set(mb) if ma[k] != mb[k])
    dev = sorted(k for k in (set(fa) | set(fb)) - set(ma) - set(mb) if fa.get(k) != fb.get(k))
    print(f"{Path(a).name}: {len(set(ma) & set(mb))} kernels compared; {len(isa)} differ in their instructions, {len(md)} in their metadata; "
          f"{len(only)} kernel symbols in one build only; {len(set(fa) - set(ma))} other device functions, {len(dev)} differ")
    for k in (only + isa + md + dev)[:20]:
        print("  differs:", k)
    bad += len(only) + len(isa) + len(md) + len(dev)
sys.exit(1 if bad else 0)
