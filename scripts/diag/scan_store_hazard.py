"""Scan gfx950 ISA listings for the store-data pattern that corrupted outputs in gemm_wreg.hip (since removed):
a buffer store of MORE than 8 bytes whose scalar-offset field holds an SGPR, followed within WINDOW vector instructions by a VALU write
of one of its data registers.  hipcc pads such a sequence to two wait states only when the field holds NO register (with an SGPR it
assumes the hardware needs none); on gfx950 a store with an SGPR there and one instruction in between read the new value for some lanes.
--flat also lists global / flat stores of more than 8 bytes (those ARE covered by the compiler's rule: expect sites whose distance is
made up of scalar instructions / branches, informational only).
   hipcc ... -save-temps=obj -c x.hip -o /tmp/isa/x.o ; python scripts/diag/scan_store_hazard.py [--flat] /tmp/isa/*gfx950.s"""
import re, sys
WINDOW = 3
st = re.compile(r"^\s*buffer_store_dword(x3|x4)\s+v\[(\d+):(\d+)\],\s*(?:v\d+|off),\s*s\[\d+:\d+\],\s*(s\d+|m0|\S+)")
# global / flat stores of more than 8 bytes: hipcc's rule applies to them whatever their address form (argv flag --flat lists them too)
gst = re.compile(r"^\s*(?:global|flat|scratch)_store_dword(x3|x4)\s+(?:v\[\d+:\d+\]|v\d+),\s*v\[(\d+):(\d+)\]")
FLAT = "--flat" in sys.argv
if FLAT: sys.argv.remove("--flat")
vdst = re.compile(r"^\s*(v_[a-z0-9_]+)\s+(v\[(\d+):(\d+)\]|v(\d+))")
total = 0
for path in sys.argv[1:]:
    lines = open(path).read().split("\n")
    kern = "?"
    for i, ln in enumerate(lines):
        if ln.endswith(":") and ln.startswith("_Z"): kern = ln[:60]
        m = st.match(ln)
        if m and not m.group(4).startswith("s"): m = None
        if m is None and FLAT:
            m = gst.match(ln)
        if not m: continue
        lo, hi = int(m.group(2)), int(m.group(3))
        seen = 0
        for j in range(i + 1, min(i + 40, len(lines))):
            t = lines[j].strip()
            if not t or t.startswith(";") or t.startswith("."): continue
            if t.startswith("s_nop"): seen += 1 + int(t.split()[1]); continue
            if t.startswith("s_"): continue                      # (scalar instructions are not wait states for this rule, conservatively skipped)
            w = vdst.match(lines[j])
            if w and not w.group(1).startswith("v_cmp"):
                a, b = (int(w.group(3)), int(w.group(4))) if w.group(3) else (int(w.group(5)), int(w.group(5)))
                if a <= hi and b >= lo:
                    print(f"{path.split('/')[-1]}:{i + 1} {kern}\n    {ln.strip()}\n    +{seen} vector instr: {t}")
                    total += 1
                    break
            seen += 1
            if seen >= WINDOW: break
print("suspect sites:", total)
