"""greyMeanAbsorptionEmission without a GPU: the fixture, the restatement and the designed inputs of the device tests.

  (a) tests/golden/greymean_case_data.json against the reference's own file (cases/pyrolysis1D/constant/radiationProperties:58-146) as
      include/ffmDictionary.H reads it through libffm_b1demo.so (b1_read_greymean): the species in file order, every coefficient -- the
      lists there carry a comment per coefficient -- EhrrCoeff and the lookUpTableFileName.  Skipped where the reference is not mounted.
  (b) the restatement (tests/greymean_ref.py) on the fixture: every species' polynomial is positive on [Tcommon, Thigh] and ends, between
      300 K and 2500 K, at the per-atm values evaluated when the model was specified (CO2 24.3 to 2.9, H2O 53.0 to 0.65, CH4 5.6 to 0.78);
      below Tcommon the result is exactly 0 (all loTcoeffs are 0).
  (c) the designed inputs of tests/test_greymean_gpu.py reach every edge of the kernel: T just below, at and above each Tcommon, both invTemp
      branches, T outside [Tlow, Thigh] on both sides, a participating species with Y == 0, a non-participating species carrying most of
      the mass, nPart == 1 and nPart == nSpecies.
  (d) the entry points are declared in include/ffm.h and exported by the library."""
import ctypes as C
import os

import numpy as np
import pytest

import greymean_ref as GM

REF_FILE = "/root/reference/cases/pyrolysis1D/constant/radiationProperties"


@pytest.mark.skipif(not os.path.exists(REF_FILE), reason="reference not mounted")
def test_fixture_equals_the_reference_file_as_the_dictionary_reader_reads_it(ffm):
    import torch  # noqa: F401
    ffm.lib()
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    lib.b1_read_greymean.restype = C.c_int
    lib.b1_read_greymean.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_int]
    out, names = np.full(200, np.nan), C.create_string_buffer(512)
    n = lib.b1_read_greymean(REF_FILE.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), len(out), names, 512)
    fx = GM.fixture()
    words = names.value.decode().split()
    assert n == 3 and words[:n] == fx["species"] == ["CO2", "H2O", "CH4"]             # file order
    assert words[n] == fx["lookUpTableFileName"] == "SpeciesTable"
    assert out[0] == fx["EhrrCoeff"]
    for j, s in enumerate(fx["species"]):
        c, row = fx["coeffs"][s], out[1 + 16 * j:1 + 16 * (j + 1)]
        assert (row[0], bool(row[1]), row[2], row[3]) == (c["Tcommon"], c["invTemp"], c["Tlow"], c["Thigh"]), s
        assert row[4:10].tolist() == c["loTcoeffs"] and row[10:16].tolist() == c["hiTcoeffs"], s
    assert np.isnan(out[1 + 16 * n])
    # the reference's dictionary names a look-up table: the class layer refuses it by name unless the caller overrides the keyword
    lib.b1_greymean_table_refusal.restype = C.c_int
    lib.b1_greymean_table_refusal.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    msg = C.create_string_buffer(512)
    assert lib.b1_greymean_table_refusal(REF_FILE.encode(), b"", msg, 512) > 0
    assert b"lookUpTableFileName SpeciesTable" in msg.value and b"not built" in msg.value
    assert lib.b1_greymean_table_refusal(REF_FILE.encode(), b"none", msg, 512) == 0 and msg.value == b""


def test_polynomials_are_positive_above_Tcommon_and_zero_below():
    fx = GM.fixture()
    ends = {"CO2": (24.3, 2.9), "H2O": (53.0, 0.65), "CH4": (5.6, 0.78)}
    for s in fx["species"]:
        c = fx["coeffs"][s]
        T = np.linspace(c["Tcommon"], c["Thigh"], 4401)
        k = GM.polynomial(c, T)
        assert np.all(k > 0), (s, k.min())
        lo, hi = ends[s]
        assert abs(k[0] - lo) < 0.05 * lo and abs(k[-1] - hi) < 0.05 * hi, (s, k[0], k[-1])
        below = GM.polynomial(c, np.array([c["Tlow"], np.nextafter(c["Tcommon"], 0.0)]))
        assert np.all(below == 0.0) and not np.signbit(below).any()
    # the mixture: a > 0 in a hot product mixture, exactly 0 in cold air with products
    species = ["CH4", "O2", "N2", "H2O", "CO2"]
    Y = [np.array([y, y]) for y in (0.01, 0.1, 0.7, 0.09, 0.1)]
    a = GM.aCont(species, GM.W, fx["coeffs"], fx["species"], Y, np.full(2, 101325.0), np.array([1500.0, 290.0]))
    assert a[0] > 0.1 and a[1] == 0.0


def test_designed_inputs_reach_every_edge():
    co = GM.edge_coeffs()
    order = GM.fixture()["species"]
    assert {co[s]["invTemp"] for s in order} == {True, False}                          # both invTemp branches
    assert any(any(co[s]["loTcoeffs"]) for s in order)                                 # a live low-temperature set
    Y, p, T, marks = GM.edge_inputs(1027)
    for tc in {co[s]["Tcommon"] for s in order}:
        assert (T == tc).any() and (T == np.nextafter(tc, 0.0)).any() and (T == np.nextafter(tc, 1e9)).any()
    assert all((T < co[s]["Tlow"]).any() and (T > co[s]["Thigh"]).any() for s in order)
    # a T that only CH4's narrower range excludes: the flag is per species
    assert ((T < co["CH4"]["Tlow"]) & (T >= co["CO2"]["Tlow"])).any() and ((T > co["CH4"]["Thigh"]) & (T <= co["CO2"]["Thigh"])).any()
    assert GM.outside(co, order, T)
    Yi, pi, Ti, _ = GM.edge_inputs(1027, in_range=True)
    assert not GM.outside(co, order, Ti)
    iz, im = marks["zeroY"], marks["mostlyN2"]
    assert Y[GM.SPECIES5.index("CO2")][iz] == 0.0 and "CO2" in order
    assert Y[GM.SPECIES5.index("N2")][im] > 0.95 and "N2" not in order
    assert np.allclose(np.sum(Y, axis=0), 1.0, atol=1e-14)
    # the restatement itself at the edges: the switch is `T < Tcommon`, so T == Tcommon takes the high set
    a = GM.aCont(GM.SPECIES5, GM.W, co, order, Y, p, T)
    assert np.isfinite(a).all() and a[marks["below300"]] != a[marks["at300"]]
    one = GM.aCont(GM.SPECIES5, GM.W, co, ["CH4"], Y, p, T)
    assert one[marks["below650"]] != one[marks["at650"]]
    assert GM.polynomial(co["CH4"], np.array([650.0]))[0] == GM.polynomial(dict(co["CH4"], Tcommon=0.0), np.array([650.0]))[0]
    # the order of the terms shows in the sum's rounding somewhere on these inputs: a kernel that summed in another order would be caught
    rev = GM.aCont(GM.SPECIES5, GM.W, co, order[::-1], Y, p, T)
    assert (rev != a).any() and np.allclose(rev, a, rtol=1e-14)


def test_comments_inside_lists_and_what_the_reader_leaves_alone(ffm, tmp_path):
    """the token reader of include/ffmDictionary.H drops a comment inside a parenthesised list only where it starts an item (after white
    space or a parenthesis): nested lists keep their structure, a path or URL inside a list keeps its slashes, and outside parentheses a
    token with // in it is read as before"""
    import torch  # noqa: F401
    ffm.lib()
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    lib.b1_dict_lookup.restype = C.c_int
    lib.b1_dict_lookup.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    f = tmp_path / "dict"
    f.write_text("FoamFile { version 2.0; }\n"
                 "plain (1 2 3);\n"
                 "commented\n(\n    1 // one (+/-) )\n    2 /* two ( */\n    3// no blank before: still an item start? no\n);\n"
                 "nested ( (0 0.03) // first pair\n (60 /* mid */ 0.03) ( (1 2) (3 4) ) );\n"
                 "files (http://host/a//b c//d /*x*/ e);\n"
                 "outside a//b;\n"
                 "after 7;\n")

    def look(key):
        buf = C.create_string_buffer(512)
        assert lib.b1_dict_lookup(str(f).encode(), key.encode(), buf, 512) >= 0, key
        return buf.value.decode()
    assert look("plain") == "(1 2 3)"
    assert look("commented").split() == ["(", "1", "2", "3//", "no", "blank", "before:", "still", "an", "item", "start?", "no", ")"]
    assert look("nested").split() == ["(", "(0", "0.03)", "(60", "0.03)", "(", "(1", "2)", "(3", "4)", ")", ")"]
    assert look("files").split() == ["(http://host/a//b", "c//d", "e)"]
    assert look("outside") == "a//b" and look("after") == "7"


NEW_SYMBOLS = ["ffm_greymean_create", "ffm_greymean_destroy", "ffm_greymean_a_d", "ffm_greymean_E_d",
               "ffm_fvdom_ray_assemble_v_d", "ffm_radiation_sh_v_d", "ffm_radiation_sh_greymean_d", "ffm_plume_set_absorption_emission"]


def test_the_entry_points_are_declared_and_exported(ffm):
    declared = ffm.declared_symbols()
    ffm.build()
    exported = ffm.exported_symbols()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffm.h")).read()
    for name in NEW_SYMBOLS:
        # (declared_symbols() lists lower-case names only: ffm_greymean_E_d, like ffm_thermo_Cp_d, is looked up in the header itself)
        assert name in declared or ("int %s(" % name) in header, name
        assert name in exported, name
