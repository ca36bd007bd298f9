"""The assertions more than one test module makes, stated once: bit-for-bit comparisons in their two meanings, a refused call, a header against the
library's exports, and a struct's layout as gcc sees it. A support module beside the tests, like sample_corners.py: imported, never collected."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_strict(a, b):
    """Equal to the last bit: a NaN equals only a NaN of the same payload, +0 and -0 differ."""
    a, b = _u32(a), _u32(b)
    return a.shape == b.shape and bool((a == b).all())


def same_bits(a, b):
    """Equal to the last bit (two NaNs count as equal, +0 and -0 do not)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def differing(a, b, per_pixel=False):
    """(count, the first three positions) of the words whose bits differ; per_pixel: of the pixels (axis 2 reduced) with such a word."""
    bad = _u32(a) != _u32(b)
    if per_pixel:
        bad = bad.any(axis=2)
    return int(bad.sum()), np.argwhere(bad)[:3].tolist()


def refused(kz, fn, code, *words):
    """fn() raises KzError with `code`, and its message holds every one of `words`."""
    with pytest.raises(kz.abi.KzError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def _exported(path):
    return set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)))


def header_surface(kz, header, exports, count, disjoint_from, older, words, resolve=True, dev_required=False):
    """A header that is a surface of its own. What it declares is `exports` (a list of kz.abi, `count` long) and is exported by the product library and by the
    development library (which must exist if dev_required, and is looked at only if it exists otherwise); every symbol resolves (resolve); it shares nothing with
    the lists of disjoint_from; none of `words` appears, in any case, in the headers `older` (paths below the repository's root; a directory stands for every file
    in it); the ABI version is 6.
    Returns (the library, the header's text) for the caller's own checks of constants."""
    a = kz.abi
    lib = a.load_library()
    src = open(os.path.join(ROOT, header)).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?(kz_[a-z0-9_]+)\s*\(", src, re.M))
    assert declared == set(exports) and len(exports) == count, declared ^ set(exports)
    exported = _exported(a.LIB_PATH)
    assert declared <= exported, declared - exported
    if dev_required:
        assert os.path.exists(a.DEV_LIB_PATH)
    if os.path.exists(a.DEV_LIB_PATH):
        dev = _exported(a.DEV_LIB_PATH)
        assert declared <= dev, declared - dev
    if resolve:
        for sym in declared:
            assert getattr(lib, sym) is not None
    for other in disjoint_from:
        assert not (declared & set(other)), declared & set(other)
    files = []
    for n in older:
        files += [n + "/" + x for x in sorted(os.listdir(os.path.join(ROOT, n)))] if os.path.isdir(os.path.join(ROOT, n)) else [n]
    for name in files:
        text = open(os.path.join(ROOT, name)).read().lower()
        for word in words:
            assert word not in text, (name, word)
    assert lib.kz_abi_version() == a.KZ_ABI_VERSION == 6
    return lib, src


def c_layout(tmp_path, header, expressions, include="include"):
    """What gcc makes of `expressions` (sizeof / offsetof print as %zu, anything else as %u) with `header` included from the directory `include`: a C program is
    written to tmp_path, compiled and run, and the tokens it printed are returned."""
    fmt = " ".join("%zu" if e.startswith(("sizeof", "offsetof")) else "%u" for e in expressions)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (header, fmt, ", ".join(expressions)))
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, include), str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).split()


def all_samples_equal_the_oracle(kz, O, sc, desc, stride=1):
    """(every sample of every stride-th pixel has the oracle's bits, the number of samples that do not)."""
    w, h, n = desc.camera["width"], desc.camera["height"], sc.sample_count
    yy, xx, ii = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), np.arange(n), indexing="ij")
    pxy, idx = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)
    g, c = sc.render_samples(pxy, idx), O.OracleScene(desc).render_samples(pxy, idx)
    assert np.abs(c[:, 2:]).max() > 0
    return same_bits(g, c), int((g.view(np.uint32) != c.view(np.uint32)).any(axis=1).sum())


def tie_bracket(ora, sc, desc, tol=1e-3):
    """The reference's shadow loop has a built-in tie (integrator.cpp:262-278): after walking through an invisible light the far end becomes maxt - t
    while the origin moved on by t + eps, so the remaining segment ends exactly ON the sampled light and whether a VISIBLE sampled light then
    occludes itself is decided by the last bit of everything upstream - in the reference as in any restatement of it. Where the upstream
    arithmetic is only equal to an ulp (libm sin / cos on the lens or in a BSDF sample) the oracle and the HIP path decide some of these ties
    differently; both are roundings of the same reference. The oracle renders the two extreme resolutions (every tie occluded / none) and every
    rounding must lie between them SAMPLE by sample (a pixel would not do: filters with negative lobes are not monotone). Returns
    (share of HIP samples outside the bracket by more than tol, number of samples with an open bracket). A closed bracket is the literal oracle's
    value, so the first number is the usual per-sample parity there."""
    w, h, n = desc.camera["width"], desc.camera["height"], sc.sample_count
    yy, xx, ii = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), indexing="ij")
    pxy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)
    idx = ii.ravel().astype(np.uint32)
    g = sc.render_samples(pxy, idx)[:, 2:5]
    c = ora.render_samples(pxy, idx)[:, 2:5]
    ora.set_tie_mode(+1); lo = ora.render_samples(pxy, idx)[:, 2:5]
    ora.set_tie_mode(-1); hi = ora.render_samples(pxy, idx)[:, 2:5]
    ora.set_tie_mode(0)
    slack = tol * (1.0 + np.abs(hi))
    assert (lo <= c + slack).all() and (c <= hi + slack).all()
    outside = ~((g >= lo - slack) & (g <= hi + slack)).all(axis=1)
    return float(outside.mean()), int(((hi - lo) > slack).any(axis=1).sum())
