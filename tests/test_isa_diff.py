"""tools/isa_diff.py on hand-written assembly: what it strips, what it reports."""
import importlib.util
from pathlib import Path

_spec = importlib.util.spec_from_file_location("isa_diff", Path(__file__).resolve().parents[1] / "tools" / "isa_diff.py")
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def _kernel(name: str, index: int, body: str, vgprs: int = 8) -> str:
    return f"""\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
{body}
\ts_cbranch_execz .LBB{index}_2
.LBB{index}_2:                          ; %exit
\ts_endpgm
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
"""


def _write(d: Path, stem: str, text: str) -> Path:
    d.mkdir(exist_ok=True)
    p = d / f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s"
    p.write_text(text)
    return p


def test_moved_kernels_compare_equal_and_copies_need_the_flag(tmp_path, capsys):
    a = "\tv_add_f32_e32 v0, v1, v2 ; a comment"
    b = "\tv_mul_f32_e32 v0, v1, v2"
    _write(tmp_path / "old", "one", _kernel("ka", 0, a) + _kernel("kb", 1, b) + _kernel("fin", 2, b))
    # kb first in its file (other label numbers), fin compiled into both files
    _write(tmp_path / "new", "x", _kernel("ka", 0, a.split(";")[0]) + _kernel("fin", 1, b))
    _write(tmp_path / "new", "y", _kernel("kb", 0, b) + _kernel("fin", 1, b))
    args = ["--old", str(tmp_path / "old"), "--new", str(tmp_path / "new")]
    assert isa_diff.main(args) == 1 and "2 copies in new" in capsys.readouterr().out
    assert isa_diff.main(args + ["--allow-dup", "fin"]) == 0
    assert "compared 3 (4 copies): 3 identical, 0 differing" in capsys.readouterr().out


def test_reports_changed_instruction_changed_descriptor_and_missing_kernel(tmp_path, capsys):
    a = "\tv_add_f32_e32 v0, v1, v2"
    old = _write(tmp_path, "old", _kernel("ka", 0, a) + _kernel("kb", 1, a) + _kernel("kc", 2, a))
    new = _write(tmp_path, "new", _kernel("ka", 0, a.replace("v2", "v3")) + _kernel("kb", 1, a, vgprs=9))
    assert isa_diff.main(["--old", str(old), "--new", str(new)]) == 1
    out = capsys.readouterr().out
    assert "only in old: kc" in out and "differs (new-hip-amdgcn-amd-amdhsa-gfx950.s): ka" in out
    assert "+ v_add_f32_e32 v0, v1, v3" in out and "+ .amdhsa_next_free_vgpr 9" in out
    assert "1 identical" not in out and "0 identical, 2 differing" in out
