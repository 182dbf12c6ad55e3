"""Writes tests/golden/pyrolysis1d_case_data.json: the model selections and numeric case data of the reference's pyrolysis1D case
(BASELINE config 1) that the config-1 tests need -- the pyrolysis model and its switches, the solids, the reaction, the surface
radiation data, the laplacian schemes of the panel region, the two patches of T (fixedIncidentRadiation on the exposed face,
constHTemperature at the back), the extrusion, the time controls and the sampling interval of the function objects -- parsed from
the case files where they lie (/root/reference/cases/pyrolysis1D).  Data only: keywords and numbers, no text of the reference.
Run from the repository root:  python tests/golden/make_pyrolysis1d_case_data.py"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_wallfire_case_data import num, parse as parse_file      # noqa: E402  the dictionary parser; an absolute path overrides its case

CASE = "/root/reference/cases/pyrolysis1D"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pyrolysis1d_case_data.json")


def parse(path):
    return parse_file(os.path.join(CASE, path))


def build():
    pz = parse("constant/pyrolysisZones")["pyrolysis"]
    model = pz["pyrolysisModel"]
    co = pz[model + "Coeffs"]
    srad = parse("constant/panelRegion/radiationProperties")
    sae = srad[srad["absorptionEmissionModel"] + "Coeffs"]
    th = parse("constant/panelRegion/thermo.solid")
    rx = parse("constant/panelRegion/reactions")
    reaction = list(rx["reactions"].values())[0]
    order = float(re.match(r"\s*(\w+)\^([0-9.eE+-]+)", reaction["reaction"].strip('"')).group(2))
    fvs = parse("system/panelRegion/fvSchemes")
    sch = fvs["laplacianSchemes"]
    T0 = parse("0/panelRegion/T")
    back = T0["boundaryField"]["panel_top"]
    face = T0["boundaryField"]["region0_to_panelRegion_panel"]
    qr = parse("0/panelRegion/qr")["boundaryField"]
    cd = parse("system/controlDict")
    ex = parse("system/extrudeToRegionMeshDict")
    ac = parse("constant/additionalControls")
    solid = lambda n: dict(rho=num(th[n]["equationOfState"]["rho"]), Cp=num(th[n]["thermodynamics"]["Cp"]), Hf=num(th[n]["thermodynamics"]["Hf"]),
                           kappa=num(th[n]["transport"]["kappa"]), absorptivity=num(sae[n]["absorptivity"]), emissivity=num(sae[n]["emissivity"]))
    probes = cd["functions"]["probes"]
    return {
        "source": "cases/pyrolysis1D: constant/{pyrolysisZones,additionalControls}, constant/panelRegion/{radiationProperties,thermo.solid,reactions}, "
                  "system/panelRegion/fvSchemes, 0/panelRegion/{T,qr}, system/{controlDict,extrudeToRegionMeshDict}",
        "solvePrimaryRegion": ac["solvePrimaryRegion"],
        "pyrolysis": {"pyrolysisModel": model, "gasHSource": co["gasHSource"], "qrHSource": co["qrHSource"], "moveMesh": co["moveMesh"],
                      "useChemistrySolvers": co["useChemistrySolvers"], "nLayers": int(num(ex["nLayers"])), "thickness": num(ex["linearNormalCoeffs"]["thickness"])},
        "solids": {"wood": solid("wood"), "char": solid("char")},
        "absorptionEmissionModel": srad["absorptionEmissionModel"],
        "reaction": {"A": num(reaction["A"]), "Ta": num(reaction["Ta"]), "Tcrit": num(reaction["Tcrit"]), "order": order},
        "panelSchemes": {"laplacian(kappa,T)": sch["laplacian(kappa,T)"][1], "laplacian(thermo:alpha,h)": sch["laplacian(thermo:alpha,h)"][1],
                         "interpolationDefault": fvs["interpolationSchemes"]["default"]},
        "panelT": {"internalField": num(T0["internalField"]), "back": {"type": back["type"], "Tinf": num(back["Tinf"]), "h": num(back["h"])},
                   "exposed": {"type": face["type"], "kappaMethod": face["kappaMethod"], "QrIncident": num(face["QrIncident"])}},
        "panelQr": {"back": qr["panel_top"]["type"], "exposed": qr["region0_to_panelRegion_panel"]["type"]},
        "controls": {"deltaT": num(cd["deltaT"]), "endTime": num(cd["endTime"]), "adjustTimeStep": cd["adjustTimeStep"],
                     "sampleInterval": int(num(probes["writeInterval"])), "sampledFields": probes["fields"].strip("()").split()},
    }


def dumps():
    return json.dumps(build(), indent=1)


if __name__ == "__main__":
    open(OUT, "w").write(dumps())
    print("wrote", OUT)
