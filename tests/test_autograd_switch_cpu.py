"""Host-side checks of the opt-in differentiable mode (no device needed): the switch's default, the loss entries' grad mode with the switch
off and on, and the C entry's binding."""
import torch

from cmdgen_amd.equivariant_diffusion.en_diffusion import no_grad_unless_differentiable


class _Dyn:
    differentiable = False


class _Loss:
    def __init__(self):
        self.dynamics = _Dyn()

    @no_grad_unless_differentiable
    def forward(self):
        return torch.is_grad_enabled()


def test_loss_entries_run_without_grad_unless_switched_on():
    m = _Loss()
    assert m.forward() is False                      # default: as @torch.no_grad()
    m.dynamics.differentiable = True
    assert m.forward() is True                       # switch on, grad mode on: autograd builds the loss
    with torch.no_grad():
        assert m.forward() is False                  # switch on, grad mode off: stays off
    assert torch.is_grad_enabled()


def test_module_switch_defaults_off_and_passes_through():
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    dyn = EGNNDynamics(phar_nf=8, residue_nf=20, n_dims=3, joint_nf=16, hidden_nf=64, n_layers=1, update_pocket_coords=False)
    assert dyn.differentiable is False
    assert dyn.set_differentiable(True) is dyn and dyn.differentiable is True
    dyn.set_differentiable(False)
    assert dyn.differentiable is False


def test_input_gradient_entry_is_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    assert lib.cmdgen_train_backward_inputs.argtypes is not None
    assert hasattr(hip_backend.Handle, 'train_backward_inputs')
