"""Record the layout of the reference's ``GATNetHeadsChanged3LayersEmbeddingDim256Entropy``
(models.py:1112-1148): state_dict keys and shapes, parameter count, child order and ``alpha``.

    python tests/golden/make_entropy_layout.py <reference tree>

Imports the reference ``models.py`` with the stand-ins of ``tests/golden/_stubs`` (as make_golden.py
does) and only constructs the class: no GAT arithmetic runs.  Only data is written."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "GATNetHeadsChanged3LayersEmbeddingDim256Entropy"


def main(ref):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.join(HERE, "_stubs"))
    sys.path.insert(0, ref)
    import models as ref_models
    torch.manual_seed(0)
    m = getattr(ref_models, NAME)()
    sd = m.state_dict()
    out = {"keys": list(sd), "shapes": [list(v.shape) for v in sd.values()],
           "parameters": sum(p.numel() for p in m.parameters()), "alpha": m.alpha,
           "children": [n for n, _ in m.named_children()]}
    with open(os.path.join(HERE, f"layout_{NAME}.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(out["parameters"], out["keys"])


if __name__ == "__main__":
    main(sys.argv[1])
