#!/usr/bin/env python3
"""One row per kernel from the remarks of  make -C panmap_amd/csrc -Otarget EXTRA=-Rpass-analysis=kernel-resource-usage :
translation unit, kernel, SGPRs, VGPRs, AGPRs, scratch bytes per lane, dynamic stack, occupancy, spills, LDS.  The project's
kernels are listed in full; the rocPRIM template kernels fold into one row per translation unit and kind (their number and
the SHA-1 of their sorted rows, each kernel named by the SHA-1 of its mangled name).  Source positions are left out, so
host code that moves a kernel down the file changes nothing.   tools/kernel_resources.py build.log > rows.txt"""
import hashlib, re, subprocess, sys

FIELDS = [("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Dynamic Stack", "dynstack"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"), ("LDS Size [bytes/block]", "LDS")]
remark = re.compile(r"^(\S+?):\d+:\d+: remark:\s+(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]")

compile_line = re.compile(r"hipcc .* -c (\S+\.hip) -o ")   # -Otarget keeps a translation unit's remarks behind its command
kernels, cur, tu = [], None, "?"
for line in open(sys.argv[1], errors="replace"):
    c = compile_line.search(line)
    if c:
        tu = c.group(1)
    m = remark.match(line)
    if not m:
        continue
    unit, key, value = m.groups()
    if key == "Function Name":
        cur = {"unit": tu, "name": value}
        kernels.append(cur)
    elif cur is not None:
        cur[key] = value

names = sorted({k["name"] for k in kernels})
plain = dict(zip(names, subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))

own, folded = [], {}
for k in kernels:
    row = " ".join("%s=%s" % (short, k.get(long, "?")) for long, short in FIELDS)
    unit, name = k["unit"], plain[k["name"]].replace("(anonymous namespace)::", "")
    m = re.match(r"rocprim::(?:ROCPRIM_\w+::)?detail::(\w+?)_kernel", name) or re.match(r"rocprim::(?:ROCPRIM_\w+::)?detail::(\w+)", name)
    if m:
        folded.setdefault((unit, m.group(1)), []).append(hashlib.sha1(k["name"].encode()).hexdigest() + " " + row)
    else:
        own.append("%s %s %s" % (unit, name, row))
for r in sorted(own):
    print(r)
for (unit, kind), rows in sorted(folded.items()):
    print("%s rocprim:%s %d kernels, sha1 of their sorted rows %s" % (unit, kind, len(rows), hashlib.sha1("\n".join(sorted(rows)).encode()).hexdigest()))
