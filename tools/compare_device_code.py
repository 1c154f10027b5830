#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds, kernel by kernel (read-only on both directories).

Build each tree with the Makefile's flags plus -save-temps=obj into a directory of its own, then
    python3 tools/compare_device_code.py OLD_DIR NEW_DIR
Every FUNC symbol's bytes and every kernel descriptor (<kernel>.kd, bytes 16..23 masked: the code-entry offset moves with
the layout) of all *-gfx950.out device objects are compared by symbol name over the union of the translation units, so a
kernel may move between files.  Exit status 0: same symbols, same bytes.

A kernel that calls a function the compiler did not inline (`s_getpc_b64` + `@rel32`) carries the distance to it in its linked
bytes, and that distance changes when a kernel that lay between the two moves to another file.  `--relocatable` compares the
*-gfx950.o objects instead, in which such a call is still a relocation: use it to tell a moved neighbour from changed code."""
import glob, os, re, subprocess, sys

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def symbols(directory, suffix="-gfx950.out"):
    out, per_file = {}, {}
    for path in sorted(glob.glob(os.path.join(directory, "*" + suffix))):
        text = subprocess.run([READELF, "-sW", "-S", path], check=True, capture_output=True, text=True).stdout
        blob = open(path, "rb").read()
        sec = {int(m[1]): (int(m[2], 16), int(m[3], 16))  # index -> (address, file offset)
               for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", text, re.M)}
        funcs = set()
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", text, re.M):
            value, size, kind, ndx, name = int(m[1], 16), int(m[2]), m[3], int(m[4]), m[5]
            if kind == "OBJECT" and not name.endswith(".kd"):
                continue
            addr, off = sec[ndx]
            data = bytearray(blob[off + value - addr: off + value - addr + size])
            if kind == "OBJECT":
                data[16:24] = bytes(8)
            if out.setdefault(name, bytes(data)) != bytes(data):
                print(f"DIFFERENT COPIES of {name} inside {directory}")
                out[name] = b""
            if kind == "FUNC":
                funcs.add(name)
        per_file[os.path.basename(path).split("-hip-")[0]] = len(funcs)
    return out, per_file


def main(old_dir, new_dir, suffix="-gfx950.out"):
    (old, old_files), (new, new_files) = symbols(old_dir, suffix), symbols(new_dir, suffix)
    for label, files in (("old", old_files), ("new", new_files)):
        print(f"{label}: " + ", ".join(f"{k} {v}" for k, v in files.items()))
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for title, names in (("only in old", gone), ("only in new", added), ("bytes differ", differ)):
        for k in names:
            print(f"{title}: {k}")
    funcs = sum(1 for k in new if not k.endswith(".kd"))
    print(f"{funcs} code symbols, {len(new) - funcs} descriptors; only in old {len(gone)}, only in new {len(added)}, differ {len(differ)}")
    return 1 if gone or added or differ else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--relocatable"]
    sys.exit(main(args[0], args[1], "-gfx950.o" if "--relocatable" in sys.argv else "-gfx950.out"))
