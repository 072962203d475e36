"""chain_ref.run_chain on the CPU: what the loop itself owes beyond its adapters (their tests are test_cond_inpaint_cpu, test_edit_cpu,
test_multi_pocket_cpu, test_multi_edit_cpu, test_restraint_cpu, test_restrained_edit_cpu) - it refuses the combination of parts that no
chain defines."""
import numpy as np
import pytest

import multi_pocket_cases as mc
from chain_ref import run_chain


def test_groups_with_a_guide_part_are_refused():
    """No device chain guides a grouped latent, and whose pocket shift the energy would see is not defined: the loop must not define it."""
    case = mc.PAIRS
    pb = mc.member_pockets(case)
    groups = dict(group_sizes=case.group_sizes, weights=mc.weights_of(case))
    guide = dict(rec=np.zeros(0), clash_r=3.0, clash_k=1.0, scale=1.0, max_shift=1.0, guide_below=1.0)
    with pytest.raises(NotImplementedError, match='groups with a guide part'):
        run_chain(mc.params(), mc.config().as_dict(), mc.pocket_dict(pb), num_nodes_phar=case.nph, groups=groups, guide=guide, timesteps=2)
