#!/usr/bin/env python3
"""Are the kernels of two gfx950 code objects the same?  usage: isa_same.py a.elf b.elf

The inputs are device code objects (hipcc ... --cuda-device-only --no-gpu-bundle-output -c).  For every
kernel symbol (a FUNC with a <name>.kd descriptor) the two sides are compared on
  code  the bytes [value, value + size) of .text;
  kd    the 64-byte kernel descriptor, its KERNEL_CODE_ENTRY_BYTE_OFFSET aside: that field is the distance
        from the descriptor to the code, checked on each side to point at the kernel's own symbol;
  meta  the kernel's amdhsa.kernels entry (registers, spills, LDS, scratch, arguments).
Per symbol, not per section: moving a definition may reorder .text without changing any kernel.  One line
per kernel; exit status 1 on any difference or a kernel on one side only.  Needs llvm-readelf,
llvm-objcopy and llvm-readobj (ROCM, default /opt/rocm, lib/llvm/bin), no GPU."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin")
ENTRY = slice(16, 24)  # KERNEL_CODE_ENTRY_BYTE_OFFSET in the descriptor


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def section(elf, name, tmp):
    """(address, bytes) of section `name`"""
    for line in run("llvm-readelf", "-SW", elf).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s", line)
        if m and m.group(1) == name:
            out = os.path.join(tmp, "sec")
            run("llvm-objcopy", "--dump-section", "%s=%s" % (name, out), elf, os.path.join(tmp, "copy"))
            return int(m.group(2), 16), open(out, "rb").read()
    raise SystemExit("%s: no %s section" % (elf, name))


def metadata(elf):
    """kernel symbol -> its amdhsa.kernels entry, as text"""
    notes = run("llvm-readobj", "--notes", elf)
    notes = notes[notes.find("amdhsa.kernels:"):]
    notes = re.split(r"\n\S", notes, maxsplit=1)[0]  # up to the next top-level key (amdhsa.target, ...)
    out = {}
    for block in re.split(r"\n  - ", notes)[1:]:
        m = re.search(r"^\s+\.symbol:\s+'?([^'\s]+?)'?$", block, flags=re.M)
        if m:
            out[m.group(1)[:-3] if m.group(1).endswith(".kd") else m.group(1)] = block.rstrip()
    return out


def kernels(elf):
    """kernel symbol -> (code bytes, descriptor with the entry offset zeroed, entry offset ok, metadata)"""
    syms = {}
    for line in run("llvm-readelf", "-sW", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            syms[f[7]] = (int(f[1], 16), int(f[2], 0), f[3])
    with tempfile.TemporaryDirectory() as tmp:
        taddr, text = section(elf, ".text", tmp)
        raddr, rodata = section(elf, ".rodata", tmp)
    meta = metadata(elf)
    out = {}
    for name, (val, size, kind) in syms.items():
        kd = syms.get(name + ".kd")
        if kind != "FUNC" or not kd:
            continue
        code = text[val - taddr:val - taddr + size]
        desc = rodata[kd[0] - raddr:kd[0] - raddr + 64]
        if len(code) != size or len(desc) != 64:
            raise SystemExit("%s: %s lies outside its section" % (elf, name))
        entry_ok = kd[0] + int.from_bytes(desc[ENTRY], "little", signed=True) == val
        out[name] = (code, desc[:16] + bytes(8) + desc[24:], entry_ok, meta.get(name))
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "ONLY IN " + sys.argv[2 if name in b else 1]
        else:
            (ca, da, ea, ma), (cb, db, eb, mb) = a[name], b[name]
            diff = [what for what, same in (("code", ca == cb), ("kd", da == db and ea and eb),
                                            ("meta", ma == mb and ma is not None)) if not same]
            verdict = "DIFFERENT: " + " ".join(diff) if diff else "same (%d code bytes)" % len(a[name][0])
        bad += not verdict.startswith("same")
        print(name, verdict)
    print("%d kernels, %d differ" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
