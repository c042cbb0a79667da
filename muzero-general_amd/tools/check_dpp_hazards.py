"""
No-GPU check of the hand-written 64-bit DPP instructions (csrc/mzx_fused_fc.h: add_bcast_d / dpp_ready_d) on the
cross-compiled ISA of the whole library, and the static counts DESIGN.md section 4.2b quotes.

    python muzero-general_amd/tools/check_dpp_hazards.py            # compiles csrc/mzx_lib.cpp with DESIGN.md's command (minutes)
    python muzero-general_amd/tools/check_dpp_hazards.py mzx_lib.s  # reads an ISA file made by that command

add_bcast_d is an asm statement, so hipcc does not see its hazard: a VALU write of the DPP source needs two wait states before
the DPP read.  dpp_ready_d puts them behind the instruction that makes the value, once; that only holds while the compiler
places no copy of the value between the two.  For every v_fmac_f64_dpp of every kernel this script asserts that neither of
the two instructions in front of it (an s_nop N counts as N + 1) writes its DPP source pair, and that no label lies within
them (a branch could arrive there from an instruction that does).  Exit status 1 on a finding.  Run it after a compiler
update or an edit to the value chain.

It also prints, for fc2_search_kernel<SmallNetCartpole, 2, false, false>, the counts of the simulation loop: the natural
loop (its out-of-line blocks included) and the first-chunk path (header .. the first back edge behind the network's block).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COMMAND = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-S", "-x", "hip",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "muzero-general_amd", "csrc", "mzx_lib.cpp")]
PRODUCT = ("fc2_search_kernel", "SmallNet", "ELi2ELb0ELb0E")
COUNTED = (("v_mov_b32_dpp", "v_mov_b32_dpp"), ("v_mov_b64_dpp", "v_mov_b64_dpp"), ("v_fmac_f64_dpp", "v_fmac_f64_dpp"),
           ("s_nop", "s_nop"), ("v_pk_*", "v_pk_"))


def kernels(path):
    """name -> list of ('L', label) / ('I', instruction text) in text order"""
    out, body = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            body = out.setdefault(m.group(1), [])
            continue
        if body is None:
            continue
        if line.startswith(".Lfunc_end"):
            body = None
            continue
        t = line.strip()
        if re.match(r"^\.LBB\w+:", t):
            body.append(("L", t.split(":")[0]))
        elif t and not t.startswith((".", ";")):
            body.append(("I", t.split(";")[0].strip()))
    return out


def written(text):
    """(first, last) vector register an instruction writes, or None"""
    if text.startswith(("s_", "ds_write", "global_store", "buffer_store", "v_cmp")) and not text.startswith("v_cmpx"):
        return None
    m = re.match(r"\S+ v\[(\d+):(\d+)\]", text) or re.match(r"\S+ v(\d+)\b", text)
    if not m:
        return None
    lo = int(m.group(1))
    return lo, int(m.group(2)) if m.lastindex > 1 else lo


def hazards(ins):
    found = []
    for i, (kind, text) in enumerate(ins):
        if kind != "I" or not text.startswith("v_fmac_f64_dpp"):
            continue
        m = re.match(r"v_fmac_f64_dpp v\[\d+:\d+\], v\[(\d+):(\d+)\]", text)
        lo, hi = int(m.group(1)), int(m.group(2))
        states, j = 0, i - 1
        while j >= 0 and states < 2:
            k, t = ins[j]
            j -= 1
            if k == "L":
                found.append((text, "label within two wait states", t))
                break
            if t.startswith("s_nop"):
                states += int(t.split()[1]) + 1
                continue
            states += 1
            w = written(t)
            if w and not (w[1] < lo or w[0] > hi):
                found.append((text, "DPP source written by", t))
    return found


def blocks(ins):
    out, cur = [], {"labels": [], "ins": []}
    for kind, text in ins:
        if kind == "L":
            if cur["ins"]:
                out.append(cur)
                cur = {"labels": [], "ins": []}
            cur["labels"].append(text)
        else:
            cur["ins"].append(text)
            if text.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
                out.append(cur)
                cur = {"labels": [], "ins": []}
    if cur["ins"]:
        out.append(cur)
    return out


def count(B, ids):
    c = collections.OrderedDict([("instructions", 0)] + [(k, 0) for k, _ in COUNTED])
    for i in ids:
        for t in B[i]["ins"]:
            c["instructions"] += 1
            for k, prefix in COUNTED:
                if t.split()[0].startswith(prefix):
                    c[k] += 1
    return dict(c)


def loop_counts(ins):
    """The simulation loop: the widest backward branch whose span holds the network (v_fmac_f32_dpp)."""
    B = blocks(ins)
    label = {l: i for i, b in enumerate(B) for l in b["labels"]}
    target = lambda b: label.get(b["ins"][-1].split()[-1]) if b["ins"][-1].startswith(("s_cbranch", "s_branch")) else None
    succ = []
    for i, b in enumerate(B):
        last, s = b["ins"][-1], []
        if target(b) is not None:
            s.append(target(b))
        if not last.startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(B):
            s.append(i + 1)
        succ.append(s)
    best = None
    for i, b in enumerate(B):
        h = target(b)
        if h is not None and h <= i and any(t.startswith("v_fmac_f32_dpp") for k in range(h, i + 1) for t in B[k]["ins"]):
            if best is None or i - h > best[1] - best[0]:
                best = (h, i)
    header = best[0]
    tails = [i for i, b in enumerate(B) if i >= header and target(b) == header]
    pred = [[] for _ in B]
    for i, s in enumerate(succ):
        for j in s:
            pred[j].append(i)
    loop, stack = {header}, list(tails)
    while stack:            # blocks in front of the header are the launch's prologue (the rotated loop is entered in its middle)
        n = stack.pop()
        if n in loop or n < header:
            continue
        loop.add(n)
        stack.extend(pred[n])
    net = max(range(header, best[1] + 1), key=lambda i: len(B[i]["ins"]))
    first_tail = min(t for t in tails if t > net)
    return count(B, sorted(loop)), count(B, range(header, first_tail + 1))


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="mzx_isa_"), "mzx_lib.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + COMMAND + ["-o", path], check=True)
    K = kernels(path)
    n_kernels = n_fmac = 0
    bad = []
    for name, ins in K.items():
        n = sum(1 for k, t in ins if k == "I" and t.startswith("v_fmac_f64_dpp"))
        if n:
            n_kernels += 1
            n_fmac += n
            bad += [(name[:100],) + h for h in hazards(ins)]
    print(f"{n_fmac} v_fmac_f64_dpp in {n_kernels} kernels: {len(bad)} findings")
    for b in bad:
        print("  ", b)
    for name, ins in K.items():
        if all(p in name for p in PRODUCT):
            natural, first = loop_counts(ins)
            meta = open(path).read()
            at = meta.find(".amdhsa_kernel " + name)
            vgpr = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta[at:at + 4000])
            scratch = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta[at:at + 4000])
            print(name[:110])
            print("  natural loop    ", natural)
            print("  first-chunk path", first)
            print("  VGPRs", vgpr.group(1) if vgpr else "?", " scratch", scratch.group(1) if scratch else "?")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
