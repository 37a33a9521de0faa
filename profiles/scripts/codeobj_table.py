#!/usr/bin/env python3
"""Code-object metadata of the two-role IPDDP rollout kernels in two object directories, as the table of profiles/r13_inkernel_stages.md
section 3: VGPRs, SGPR / VGPR spills, LDS, scratch, occupancy (waves per SIMD from the register count) per instantiation, read from the
gfx950 code objects bundled in the inst_*.o files.  usage: codeobj_table.py <parent build dir> <build dir>"""
import re, subprocess, sys, os, glob, tempfile
def kernels(objdir):
    out = {}
    for o in sorted(glob.glob(os.path.join(objdir, "inst_*.o"))):
        with tempfile.TemporaryDirectory() as td:
            fat = os.path.join(td, "fat.bin"); co = os.path.join(td, "dev.co")
            subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", o, fat])
            subprocess.check_call(["/opt/rocm/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk)
            name = g("name").group(1)
            if "k_forward_ipddp_pcI" not in name and "k_forward_ipddp_pc_slI" not in name: continue
            out[name] = dict(v=int(g("vgpr_count").group(1)), ss=int(g("sgpr_spill_count").group(1)), vs=int(g("vgpr_spill_count").group(1)),
                             lds=int(g("group_segment_fixed_size").group(1)), scr=int(g("private_segment_fixed_size").group(1)))
    return out
def occ(v): return max(1, min(8, 512 // (((v + 7) // 8) * 8)))
def short(n):
    d = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    d = d.replace("cddp_dev::", "").replace("void ", "")
    return d[d.index("<"):d.index(">(") + 1] if ">(" in d else d
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
fmt = lambda r: "%d VGPR, %d SGPR spills, %d VGPR spills, %d B LDS, %d B scratch, occupancy %d" % (r["v"], r["ss"], r["vs"], r["lds"], r["scr"], occ(r["v"]))
print("| `k_forward_ipddp_pc<...>` | parent | this change |"); print("|---|---|---|")
strip = lambda n: re.sub(r"EEvNS_6DevBuf.*$", "", n)
bb = {strip(k): v for k, v in b.items()}
for k in sorted(a, key=short):
    r2 = bb.get(strip(k))
    print("| `%s` | %s | %s |" % (short(k), fmt(a[k]), ("same" if r2 == a[k] else fmt(r2)) if r2 else "-"))
print()
print("| `k_forward_ipddp_pc_sl<...>` (new) | figures | the plain kernel of the layout |"); print("|---|---|---|")
for k in sorted(b, key=short):
    if "pc_slI" in k:
        plain = [v for kk, v in b.items() if "pc_slI" not in kk and short(kk) == short(k)[:-2] + ", false, 1>"]
        print("| `%s` | %s | %s |" % (short(k), fmt(b[k]), fmt(plain[0]) if plain else "?"))
