"""Writes tests/golden/greymean_case_data.json: the greyMeanAbsorptionEmissionCoeffs of the reference's pyrolysis1D case
(cases/pyrolysis1D/constant/radiationProperties:58-146) -- EhrrCoeff, lookUpTableFileName and, per participating species in file order
(CO2, H2O, CH4), Tcommon, invTemp, Tlow, Thigh and the six loTcoeffs / hiTcoeffs -- parsed from the case file where it lies.  Data only:
keywords and numbers, no text of the reference.  Run from the repository root:  python tests/golden/make_greymean_case_data.py"""
import json
import os
import re

FILE = "/root/reference/cases/pyrolysis1D/constant/radiationProperties"


def build():
    txt = open(FILE).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    tok = re.findall(r'"[^"]*"|[{};()]|[^\s{};()]+', txt)
    pos = tok.index("greyMeanAbsorptionEmissionCoeffs") + 2

    def block():
        nonlocal pos
        d = {}
        while tok[pos] != "}":
            key = tok[pos]; pos += 1
            if tok[pos] == "{":
                pos += 1
                d[key] = block()
                pos += 1
            elif tok[pos] == "(":
                end = tok.index(")", pos)
                d[key] = [float(x) for x in tok[pos + 1:end]]
                pos = end + 2                                # the parenthesis and the semicolon
            else:
                d[key] = tok[pos].strip('"'); pos += 2
        return d
    co = block()
    species = [k for k, v in co.items() if isinstance(v, dict)]
    return {
        "source": "cases/pyrolysis1D/constant/radiationProperties:58-146 (greyMeanAbsorptionEmissionCoeffs)",
        "lookUpTableFileName": co["lookUpTableFileName"],
        "EhrrCoeff": float(co["EhrrCoeff"]),
        "species": species,
        "coeffs": {s: {"Tcommon": float(co[s]["Tcommon"]), "invTemp": co[s]["invTemp"] == "true", "Tlow": float(co[s]["Tlow"]),
                       "Thigh": float(co[s]["Thigh"]), "loTcoeffs": co[s]["loTcoeffs"], "hiTcoeffs": co[s]["hiTcoeffs"]} for s in species},
    }


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "greymean_case_data.json")
    json.dump(build(), open(out, "w"), indent=1)
    print("wrote", out)
