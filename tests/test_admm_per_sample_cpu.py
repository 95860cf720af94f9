"""CPU checks of the per-sample ADMM stopping mode (mgadmm_params.admm_convergence): where the new fields sit in the ABI
structs, the version the library reports, and the keyword's validation, none of which needs a GPU."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _last_field(struct_name):
    body = re.search(r"typedef struct \{([^{}]*)\} " + struct_name + ";", _header()).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    return re.findall(r"([A-Za-z_0-9]+)\s*$", decls[-1])[0], decls[-1]


def test_new_fields_are_appended_last_in_header_and_binding():
    from mgadmm import _lib
    name, decl = _last_field("mgadmm_params")
    assert name == "admm_convergence" and decl.startswith("int32_t ")
    assert _lib.Params._fields_[-1][0] == "admm_convergence"
    name, decl = _last_field("mgadmm_history")
    assert name == "n_iters_per_sample" and decl.startswith("int32_t*")
    assert _lib.History._fields_[-1][0] == "n_iters_per_sample"
    # the fields older callers know keep their offsets
    assert _lib.Params.admm_convergence.offset == _lib.Params.max_inner_iter.offset + 4
    assert _lib.History.n_iters_per_sample.offset == _lib.History.cg_beta.offset + 8


def test_enum_values_in_header_and_binding():
    from mgadmm import _lib
    m = re.search(r"typedef enum \{([^{}]*)\} mgadmm_admm_convergence_t;", _header())
    assert m, "mgadmm_admm_convergence_t is not declared"
    vals = dict(re.findall(r"(MGADMM_ADMM_[A-Z_]+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"MGADMM_ADMM_WHOLE_BATCH": "0", "MGADMM_ADMM_PER_SAMPLE": "1"}
    assert (_lib.ADMM_WHOLE_BATCH, _lib.ADMM_PER_SAMPLE) == (0, 1)
    assert _lib.Params().admm_convergence == _lib.ADMM_WHOLE_BATCH          # a zeroed struct selects the default mode


def test_version_reports_the_struct_growth():
    from mgadmm import _lib
    assert re.match(r"mgadmm 0\.3\.\d+ ", _lib.version()), _lib.version()
    assert "0.3: mgadmm_params gained admm_convergence" in open(os.path.join(ROOT, "include", "mgadmm.h")).read()


def _tiny(**kw):
    from mgadmm.ADMM import ADMM_algorithm
    cl = torch.tensor([[0, 1], [1, 0]])
    return ADMM_algorithm({"n_nodes": 2}, dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1), use_kNN=True,
                          u_sigma=1.0, d_sigma=1.0, tables=(cl, torch.tensor([[0.0, 1.0], [0.0, 1.0]])), **kw)


def test_keyword_is_validated_without_a_gpu():
    with pytest.raises(ValueError, match="admm_convergence"):
        _tiny(admm_convergence="nonsense")
    assert _tiny().admm_convergence == "whole_batch"
    blk = _tiny(admm_convergence="per_sample")
    assert blk.admm_convergence == "per_sample" and blk.n_iters_per_sample is None
    from mgadmm import _lib
    assert blk._params(torch.float32, 4).admm_convergence == _lib.ADMM_PER_SAMPLE
    blk.admm_convergence = "whole_batch"
    assert blk._params(torch.float32, 4).admm_convergence == _lib.ADMM_WHOLE_BATCH
    blk.admm_convergence = "each"            # attribute assignment is validated where the parameters are formed
    with pytest.raises(ValueError, match="admm_convergence"):
        blk._params(torch.float32, 4)
