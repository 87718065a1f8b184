"""Record the layout of the reference's six LayerNorm-tail models (models.py:321-377, :379-435, :437-526,
:528-612, :693-773, :776-832): state_dict keys and shapes, parameter count and child order.

    python tests/golden/make_layernorm_layouts.py <reference tree>

Imports the reference ``models.py`` with the stand-ins of ``tests/golden/_stubs`` (as
make_entropy_layout.py does) and only constructs the classes: no GAT arithmetic runs.  Only data is
written, one ``layout_<name>.json`` per model."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("GATNetHeadsChanged4LayersReLU_LayerNorm", "GATNetHeadsChanged4LayersLeakyReLU_LayerNorm",
         "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512", "GATNetSelectiveResiduals",
         "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals", "GATNetSelectiveResidualsUpdatedLayerNorm")


def main(ref):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.join(HERE, "_stubs"))
    sys.path.insert(0, ref)
    import models as ref_models
    for name in NAMES:
        torch.manual_seed(0)
        m = getattr(ref_models, name)()
        sd = m.state_dict()
        out = {"keys": list(sd), "shapes": [list(v.shape) for v in sd.values()],
               "parameters": sum(p.numel() for p in m.parameters()),
               "children": [n for n, _ in m.named_children()]}
        with open(os.path.join(HERE, f"layout_{name}.json"), "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(name, out["parameters"])


if __name__ == "__main__":
    main(sys.argv[1])
