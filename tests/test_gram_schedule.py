"""CPU: in the gfx950 code object of the built library, every gather-Gram
instance for k <= 64 (gram_kernel<NB <= 4, ...>) issues the row gathers of the
next 32-rating half a whole MFMA phase ahead of their first use.

The main loop of gram_wave (kernels.hip) gathers half h+1 while the matrix
cores work on half h.  Left to the machine scheduler, the eight gathers of an
iteration sank behind most of the iteration's MFMAs, so a wave had only a
quarter of the phase between issuing 512 row fetches and waiting for the
first.  This check reads the emitted code, as tests/test_asm_guards.py does:

  * in the main loop (the body of a backward branch that holds MFMAs and row
    gathers), every row gather of the iteration comes before the iteration's
    first MFMA.  A row gather is a load of NB dwords per lane: the only loads
    wider than a dword in the loop at NB >= 2 (the id / rating / bias prefetch
    loads one dword each, at most 3 per iteration).  At NB = 1, and at NB = 3
    if the rows are fetched as single dwords, every load of the loop must
    come first or be one of those at most 3 prefetch dwords;
  * the kernel's metadata shows no scratch and no spills;
  * its register count allows 3 waves per SIMD (<= 168 of the 512 unified
    VGPRs of a gfx950 SIMD, AGPRs included).
"""
import os
import re
import shutil
import subprocess

import pytest

from test_asm_guards import LLVM, SO, _gfx950_objects

MAX_VGPR_3_WAVES = 168     # 512 // 3, rounded down to the allocation granule of 8


def _kernel_meta(path):
    """{kernel name: {field: int}} from the code object's amdhsa.kernels note."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True,
                           text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if line.lstrip().startswith("- ."):      # first field of a new kernel record
            cur = {}
        if cur is None:
            continue
        cur[key] = val
        if key == "name":
            out[val] = cur
    return out


def _instructions(path):
    """{function: [(address, instruction text)]} from llvm-objdump -d."""
    asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", path], capture_output=True,
                         text=True).stdout
    out = {}
    for chunk in re.split(r"\n(?=[0-9a-f]{16} <)", asm):
        m = re.match(r"[0-9a-f]{16} <([^>]+)>:", chunk)
        if not m:
            continue
        ins = []
        for line in chunk.splitlines()[1:]:
            mm = re.match(r"\s*(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if mm:
                ins.append((int(mm.group(2), 16), mm.group(1)))
        out[m.group(1)] = ins
    return out


def _loops(ins):
    """(first, last) instruction indices of every backward-branch body."""
    at = {a: t for t, (a, _) in enumerate(ins)}
    out = []
    for t, (a, i) in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\d+)$", i)
        if not m:
            continue
        off = int(m.group(1))
        if off < 0x8000:
            continue
        target = a + 4 + (off - 0x10000) * 4
        if target in at:
            out.append((at[target], t))
    return out


def _is_load(i):
    return re.match(r"(global|buffer|flat)_load_", i) is not None


def _is_wide_load(i):
    return re.match(r"(global|buffer|flat)_load_dwordx[234]\b", i) is not None


def analyse(so):
    """Per gram_kernel<NB <= 4> instance: NB, the main loop's instruction
    texts, and the kernel's metadata."""
    found = {}
    for j, obj in enumerate(_gfx950_objects(so)):
        path = os.path.join(analyse.tmp, f"co{j}.o")
        with open(path, "wb") as f:
            f.write(obj)
        meta = _kernel_meta(path)
        for name, ins in _instructions(path).items():
            m = re.search(r"gram_kernelILi(\d+)E", name)
            if not m or int(m.group(1)) > 4:
                continue
            bodies = []
            for a, b in _loops(ins):
                body = [i for _, i in ins[a:b + 1]]
                if any(i.startswith("v_mfma") for i in body) and any(_is_load(i) for i in body):
                    bodies.append(body)
            found[name] = (int(m.group(1)), bodies, meta.get(name))
    return found


@pytest.mark.skipif(not os.path.exists(SO) or not shutil.which(f"{LLVM}/llvm-objdump"),
                    reason="library or llvm-objdump missing")
def test_gram_gathers_lead_the_mfma_phase(tmp_path):
    analyse.tmp = str(tmp_path)
    found = analyse(SO)
    # NB = 1 .. 4 x user (rhs on VALU or MFMA) / item x fused / unfused
    # (x buffer forms at NB = 4)
    assert len(found) >= 30, sorted(found)
    for name, (nb, bodies, meta) in sorted(found.items()):
        assert len(bodies) == 1, (name, len(bodies))     # the one main loop
        body = bodies[0]
        first_mfma = next(t for t, i in enumerate(body) if i.startswith("v_mfma"))
        n_mfma = sum(i.startswith("v_mfma") for i in body)
        assert n_mfma >= 6 * nb * (nb + 1) // 2, (name, n_mfma)
        wide = [t for t, i in enumerate(body) if _is_wide_load(i)]
        late = [t for t, i in enumerate(body) if _is_load(i) and t > first_mfma]
        if wide:
            assert len(wide) == 8, (name, len(wide))
            assert max(wide) < first_mfma, (name, [t - first_mfma for t in wide], n_mfma)
        else:
            assert nb in (1, 3), (name, "no wide row gathers")
            early = [t for t, i in enumerate(body) if _is_load(i) and t < first_mfma]
            assert len(early) >= 8 * nb, (name, len(early))
        assert len(late) <= 3, (name, [body[t] for t in late])
        assert meta is not None, name
        assert int(meta["private_segment_fixed_size"]) == 0, (name, meta)
        assert int(meta.get("vgpr_spill_count", 0)) == 0, (name, meta)
        assert int(meta.get("sgpr_spill_count", 0)) == 0, (name, meta)
        total = int(meta["vgpr_count"])
        assert total <= MAX_VGPR_3_WAVES, (name, total)
