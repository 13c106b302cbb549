"""Dev tool: per-kernel VGPR / SGPR / spill / scratch / LDS usage of the gfx950 code object in
build/igx_device_p*.o (reads the AMDGPU metadata notes), and its static instruction mix from the
disassembly of the same code object: all VALU (v_*), packed f32 VALU (v_pk_*_f32 and v_pk_mov_b32,
what the SLP vectoriser makes of adjacent f32 operations), register moves (v_mov_b32 / _b64 and
v_accvgpr moves), v_readlane / v_writelane (SGPR spills) and scratch instructions.
usage: kernel_resources.py [--md | --digest] [name filter] [objects...]
  --md      a markdown table (profiles/r11_kernel_resources.md) instead of one text line per kernel
  --digest  one line per symbol of each object's code object: the object, the symbol, a hash of
            its disassembled instructions (no addresses, no raw bytes, nothing behind the last
            s_endpgm) and the metadata figures; two builds have the same device code where the
            sorted outputs are equal (profiles/kernel_choice_digest.md)"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
args = sys.argv[1:]
md = "--md" in args
digest = "--digest" in args
args = [a for a in args if a not in ("--md", "--digest")]
pat = args[0] if args else ("" if digest else "k_")
objs = args[1:] or sorted(glob.glob("ignis-masterthesis_amd/build/igx_device_p*.o"))


def instruction_mix(co):
    """{mangled kernel name: counts} from llvm-objdump -d of one code object."""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    mix, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = mix.setdefault(m.group(1), dict(valu=0, pk=0, mov=0, lane=0, scratch=0))
            continue
        op = line.split()[0] if cur is not None and line.startswith(("\t", " ")) and line.split() else ""
        if op.startswith("v_"):
            cur["valu"] += 1
            if re.match(r"v_pk_\w+_f32|v_pk_mov_b32", op):
                cur["pk"] += 1
            elif op.startswith(("v_mov_b", "v_accvgpr_")):
                cur["mov"] += 1
            elif op.startswith(("v_readlane", "v_writelane")):
                cur["lane"] += 1
        elif op.startswith("scratch_"):
            cur["scratch"] += 1
    return mix


def instruction_digests(co):
    """{mangled symbol: sha1 of its instructions} from llvm-objdump -d of one code object: the
    text of each instruction without its address comment, up to the symbol's last s_endpgm
    (what follows is padding, which objdump may fold into a '...' line)."""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    body, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur.append(" ".join(line.split("//")[0].split()))
    out = {}
    for name, ins in body.items():
        ends = [k for k, i in enumerate(ins) if i.startswith("s_endpgm")]
        out[name] = hashlib.sha1("\n".join(ins[:ends[-1] + 1] if ends else ins).encode()).hexdigest()[:16]
    return out


def kernel_notes(notes):
    """(mangled name, its entry's text) per kernel of the metadata note: an entry starts at a
    list item of amdhsa.kernels (its fields are sorted, so some stand before .name)."""
    for b in re.split(r"^  - ", notes, flags=re.M)[1:]:
        m = re.search(r"^\s+\.name:\s+(\S+)", b, flags=re.M)
        if m:
            yield m.group(1), b


FIGURES = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
rows = []
with tempfile.TemporaryDirectory() as tmp:
    fat, host, co = (os.path.join(tmp, n) for n in ("fat.bin", "host.o", "dev.co"))
    for obj in objs:
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, host], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        if digest:
            figures = {name: [(re.search(r"\." + k + r":\s+(\d+)", b) or [None, "-"])[1] for k in FIGURES] for name, b in kernel_notes(notes)}
            syms = sorted(n for n in instruction_digests(co).items() if pat in n[0])
            names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in syms), capture_output=True, text=True).stdout.split("\n")
            for (n, h), dn in zip(syms, names):
                print(os.path.basename(obj), re.sub(r"^void igxh::", "", dn).split("(")[0].replace(" ", ""), h, *figures.get(n, ["-"] * len(FIGURES)))
            continue
        mix = None
        for name, b in kernel_notes(notes):
            if pat not in name:
                continue
            if mix is None:
                mix = instruction_mix(co)
            dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            g = lambda k: (re.search(r"\." + k + r":\s+(\d+)", b) or [None, "-"])[1]
            rows.append((dn, [g(k) for k in FIGURES],
                         mix.get(name, dict(valu="-", pk="-", mov="-", lane="-", scratch="-"))))

if md:
    print("| kernel | vgpr | spill | sgpr | sspill | priv | lds | VALU | v_pk_*_f32 | v_mov | v_readlane/writelane | scratch |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for dn, r, m in rows:
        short = re.sub(r"^void igxh::", "", dn).split("(")[0]
        print(f"| `{short}` | " + " | ".join(r) + f" | {m['valu']} | {m['pk']} | {m['mov']} | {m['lane']} | {m['scratch']} |")
else:
    for dn, r, m in rows:
        print(f"{dn[:70]:70s} vgpr {r[0]:>4} spill {r[1]:>3} sgpr {r[2]:>4} sspill {r[3]:>3} priv {r[4]:>4} lds {r[5]:>6} "
              f"valu {m['valu']:>6} pk {m['pk']:>5} mov {m['mov']:>5} lane {m['lane']:>4} scratch {m['scratch']:>4}")
