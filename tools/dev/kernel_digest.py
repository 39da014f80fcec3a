"""tools/dev/kernel_digest.py [--order] ct_raster.o: one line `hash mangled-name` per gfx950 kernel of an object file, the hash over
the kernel's disassembly without addresses and encodings (branch operands are relative: the text does not depend on where a kernel
was placed).  `diff` the lists of two builds to prove a host-side change left the device code alone, kernel by kernel.

The lines come sorted by name; with --order they come in the order the kernels have in the code object (the disassembly's own
order), which is what the instantiation list of csrc/ct_gconv.hip pins and what a second `diff` then proves unchanged."""
import hashlib, os, re, subprocess, sys, tempfile

args = [a for a in sys.argv[1:] if a != "--order"]
in_order = len(args) != len(sys.argv) - 1
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
with tempfile.TemporaryDirectory() as d:
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, args[0]], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co],
                         capture_output=True, text=True, check=True).stdout
cur, out = None, {}                    # (a dict keeps the order of first insertion: the disassembly's)
for line in txt.splitlines():
    m = re.match(r"^<(.+)>:$", line)
    if m:
        cur = m.group(1)
        out[cur] = hashlib.sha1()
    elif cur and line.strip():
        out[cur].update(line.split("//")[0].strip().encode() + b"\n")
for k in (out if in_order else sorted(out)):
    print(out[k].hexdigest()[:16], k)
