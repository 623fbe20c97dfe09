"""CPU-side (-m "not gpu"): the binding is read off the header (dehaze_hip._lib.parse_header, checked here on strings), and the window-side
wrappers of dehaze_hip.ops / fused make one call per op, to the `_w` entry - held against the calls of the commit that still chose
between the entry with and the entry without `_w`."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VP, CI, CL, CF, CD, CZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

# every shape include/dehaze_hip.h contains today, in one text: the guard, `extern "C"`, #defines (one with a comment; and a continued one,
# which the header does not have), block and line comments that name entries and hold `;` and `(`, (void), a prototype over three lines,
# `const float* const*`, `void**`, every scalar type and every return type
_HEADER = r"""
/* dhz_first(int a); is described here; so is dhz_never( */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define DHZ_EINVAL (-22)  /* bad argument; dhz_last_error() has the text */
#define DHZ_LONG(a, b) \
    dhz_not_an_entry(a, b);
int dhz_abi_version(void);
const char* dhz_last_error(void);
const char *dhz_build_id( void );   // dhz_commented_out(int x);
size_t dhz_bytes(int B, int64_t n, float eps, double c1, size_t have);
/* a comment
 * over lines: int dhz_in_comment(int n); */
int dhz_multi(const float* const* dw, float* const* db,
              void** comm, const uint8_t* idx, const uint64_t* pad, int n,
              void* stream);
int dhz_unnamed(int, float*);
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


def test_parse_header_on_every_shape_the_header_contains():
    from dehaze_hip import _lib
    args, rets = _lib.parse_header(_HEADER)
    assert args == {"dhz_abi_version": [], "dhz_last_error": [], "dhz_build_id": [], "dhz_bytes": [CI, CL, CF, CD, CZ],
                    "dhz_multi": [VP, VP, VP, VP, VP, CI, VP], "dhz_unnamed": [CI, VP]}
    assert rets == {"dhz_abi_version": CI, "dhz_last_error": ctypes.c_char_p, "dhz_build_id": ctypes.c_char_p, "dhz_bytes": CZ,
                    "dhz_multi": CI, "dhz_unnamed": CI}
    assert _lib.parse_header("") == ({}, {})


@pytest.mark.parametrize("text,what", [
    ("int dhz_x(unsigned long n);", "unsigned long n"),                      # a scalar type outside the table
    ("int dhz_x(int a, char c);", "char c"),
    ("int dhz_x(int n[4]);", "n[4]"),
    ("long dhz_x(int n);", "'long'"),                                        # a return type outside the table
    ("float* dhz_x(int n);", "'float*'"),
    ("int dhz_ok(int n);\nint dhz_y(int a,", "dhz_y"),                       # a prototype that is cut off: at the end of the text,
    ("int dhz_y(int a,\nint dhz_ok(int n);", "dhz_y"),                       # ... before the next one,
    ("int dhz_y(int a)\nint dhz_ok(int n);", "dhz_y"),                       # ... without its semicolon
    ("int dhz_x(int n);\nint dhz_x(int n);", "twice"),
    ("typedef int dhz_t;", "dhz_t"),                                          # whatever is no prototype at all
    ("int other(int n);", "other"),
])
def test_parse_header_never_guesses(text, what):
    from dehaze_hip import _lib
    with pytest.raises(ValueError) as e:
        _lib.parse_header(text)
    assert what in str(e.value), str(e.value)               # the message names the prototype


def test_a_missing_header_fails_the_import_loudly(tmp_path, monkeypatch):
    from dehaze_hip import _lib
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "dehaze_hip.h"))
    with pytest.raises(ImportError, match="dehaze_hip.h not found"):
        _lib._declared()


# ----------------------------------------------------------------------------- one call per window op
def _scalar_names(name):
    """names of the non-pointer parameters of `name` in include/dehaze_hip.h, in order"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dehaze_hip.h")).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, hdr).group(1)
    return [p.split()[-1] for p in params.split(",") if "*" not in p]


# entry of the parent's win = 8 route (as the log writes it) -> the `_w` entry that takes its place
_TO_W = {"ps_attn_fwd": "ps_attn_fwd_w", "ps_attn_fwd_dt": "ps_attn_fwd_w", "ps_attn_fwd_dt_pad": "ps_attn_fwd_w_pad",
         "ps_attn_bwd_dt": "ps_attn_bwd_w", "ps_attn_bwd_dt_pad": "ps_attn_bwd_w_pad", "ps_attn_bwd_parts_d": "ps_attn_bwd_parts_w",
         "ps_attn_bwd_parts": "ps_attn_bwd_parts_w", "dense_attn_fwd": "dense_attn_fwd_w", "dense_attn_bwd": "dense_attn_bwd_w",
         "bias_gather": "bias_gather_w", "bias_table_grad": "bias_table_grad_w", "shift_mask": "shift_mask_w",
         "ln_partition_fwd_dt": "ln_partition_fwd_w", "ln_partition_bwd_dt": "ln_partition_bwd_w",
         "reverse_residual_fwd_dt": "reverse_residual_fwd_w", "reverse_residual_bwd_dt": "reverse_residual_bwd_w"}


def _as_w(call, d, keep=()):
    """one logged call of the parent at win = 8 -> the call this commit must make: X_dt or plain X becomes X_w with 8 at the header's `win`
    position; the fp32-only dhz_ps_attn_fwd gains dtype 0 behind it, dhz_ps_attn_bwd_parts(B_, H) the head dim it never read"""
    name, args = call[:-1].split("(")
    if name not in _TO_W or name in keep:
        return call
    args = args.split(",")
    if name == "ps_attn_bwd_parts":
        args.append(str(d))
    names = _scalar_names("dhz_" + _TO_W[name])
    args.insert(names.index("win"), "8")
    if name == "ps_attn_fwd":
        assert names[-1] == "dtype"
        args.append("0")
    assert len(args) == len(names), (call, names)
    return _TO_W[name] + "(" + ",".join(args) + ")"


def test_window_ops_make_the_parent_commits_calls_through_the_w_entries():
    """ops.ln_partition, reverse_residual (and their token-order forms), ps_window_attention (+ _rank), dense_window_attention, each forward
    and backward, shift_mask, bias_tile, bias_table_grad, fused._bias_tile, fused._table_backward and fused._attn_bwd are driven without a
    device (tests/_window_log.py) over win 8 / 4 x fp32 / bf16 storage where the op takes it x shift mask or none x bias table or none x
    padding words or none (with and without the caller's nW).  tests/golden/window_call_log_parent.txt is the log the parent commit wrote
    for this grid (entry name + every non-pointer argument; the parent's fused._table_backward took the device as a fifth argument).
    win = 4: no line may differ.  win = 8: the parent's line after the mapping of _as_w - same arguments, same order, `win = 8` where the
    header has it - which is what a permuted B_, H, nW, d would break.  The autograd node's own `_dt` calls, which never branched,
    stay (dhz_reverse_residual_bwd_dt in fused._attn_bwd)."""
    import _window_log
    with open(os.path.join(ROOT, "tests", "golden", "window_call_log_parent.txt")) as f:
        parent = f.read().splitlines()
    got = _window_log.grid()
    assert len(parent) == len(got) == 155
    assert "ps_window_attention win8 H2 d32 mask1 table1 bf16 pad1 nWNone | bias_gather(2); ps_attn_fwd_dt_pad(192,64,8,2,4,32,1); " \
           "ps_attn_bwd_parts_d(8,2,32); ps_attn_bwd_dt_pad(192,64,192,8,2,4,32,1); bias_table_grad(6,2,0)" in parent
    want = []
    for line in parent:
        case, calls = line.split(" | ")
        if " win4 " in case + " ":
            want.append(line)
            continue
        d = int(re.search(r" d(\d+)", case).group(1)) if " d" in case else None
        keep = ("reverse_residual_bwd_dt",) if case.startswith("fused._attn_bwd") else ()
        want.append(case + " | " + "; ".join(_as_w(c, d, keep) for c in calls.split("; ")))
    assert "ps_window_attention win8 H2 d32 mask1 table1 bf16 pad1 nWNone | bias_gather_w(2,8); ps_attn_fwd_w_pad(192,64,8,2,4,32,8,1); " \
           "ps_attn_bwd_parts_w(8,2,32,8); ps_attn_bwd_w_pad(192,64,192,8,2,4,32,8,1); bias_table_grad_w(6,2,0,8)" in want
    assert "dense_window_attention win8 H1 d16 mask1 | bias_gather_w(1,8); dense_attn_fwd_w(48,16,8,1,4,16,0.25,8); " \
           "ps_attn_bwd_parts_w(8,1,16,8); dense_attn_bwd_w(48,16,48,8,1,4,16,0.25,8); bias_table_grad_w(3,1,0,8)" in want
    assert sum(line != p for line, p in zip(want, parent)) == 82 and sum(" win4 " in p.split("|")[0] for p in parent) == 73
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} of {len(want)} lines differ (parent after the mapping, now), first: {diff[:3]}"
    # no wrapper is left that names an entry of the win = 8 route in a call
    now = {c.split("(")[0] for line in got for c in line.split(" | ")[1].split("; ")}
    assert not now & (set(_TO_W) - {"reverse_residual_bwd_dt"}), now & set(_TO_W)
