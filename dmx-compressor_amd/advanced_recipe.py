"""ADVANCED-mode recipes (reference: advanced_recipe.py:14-40, 120-142): a hyperparameter generator maps a model to
{DmxModule: hyperparams}, and `applied_to(model)` enters one module context manager per entry (an ExitStack), so that leaving the
`with` block finishes every module's calibration / compression."""
from contextlib import ExitStack, contextmanager
from typing import Callable, Optional

from .nn import DmxModule

__all__ = ["DmxBaseRecipe", "DmxQuantizerCalibrationRecipe", "DmxSmoothQuantRecipe", "DmxGPTQRecipe", "DmxWandaRecipe", "DmxAWQRecipe", "DmxAWQClipRecipe", "DmxHQQRecipe", "DmxAdaRoundRecipe"]


class DmxBaseRecipe:
    """hp_gen(model) -> {module: hyperparams}; subclasses set `recipe_context_manager` (an unbound DmxModule context manager)."""

    def __init__(self, hp_gen: Callable, **kwargs):
        self.generate_hyperparams = hp_gen
        self.recipe_context_manager = None

    @contextmanager
    def applied_to(self, _model, save_checkpoint_to: Optional[str] = None):
        _hyperparams = self.generate_hyperparams(_model)
        with ExitStack() as stack:
            try:
                yield [stack.enter_context(self.recipe_context_manager(_m, _p)) for _m, _p in _hyperparams.items()]
            finally:
                if hasattr(_model, "_save_specific_layers_state_dict_and_register_urls"):
                    _model._save_specific_layers_state_dict_and_register_urls(_hyperparams.keys(), save_checkpoint_to)


class DmxQuantizerCalibrationRecipe(DmxBaseRecipe):
    """fake quantizer calibration (DmxModule.calibrating_quantizers)"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.calibrating_quantizers


class DmxSmoothQuantRecipe(DmxBaseRecipe):
    """SmoothQuant calibration (DmxModule.calibrating_smoothquant)"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.calibrating_smoothquant


class DmxGPTQRecipe(DmxBaseRecipe):
    """GPTQ (DmxModule.optimal_brain_compressing); every field of a module's DmxModuleGPTQHyperparams, `act_order` included, reaches
    OptimalBrainCompressor.apply"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.optimal_brain_compressing


class DmxWandaRecipe(DmxBaseRecipe):
    """Wanda pruning (DmxModule.wanda_pruning): hp_gen maps the model to {module: DmxWandaHyperparams}; every Linear among them with a
    weight sparseness gathers its own activation norms while the calibration batches run and is scored on exit"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.wanda_pruning


class DmxAWQRecipe(DmxBaseRecipe):
    """AWQ scaling (DmxModule.awq_scaling): hp_gen maps the model to {module: DmxAWQHyperparams}; every Linear among them with a
    smoothquant member and a weight cast gathers its own input statistics while the calibration batches run; on exit it searches its
    per-input-channel scale and hands it to its SmoothQuant"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.awq_scaling


class DmxAWQClipRecipe(DmxBaseRecipe):
    """AWQ weight clipping (DmxModule.awq_clipping): hp_gen maps the model to {module: DmxAWQClipHyperparams}; the calibration forwards
    run inside the context, and on exit every Linear among them has its weight clamped group by group (ops.awq_clip)"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.awq_clipping


class DmxHQQRecipe(DmxBaseRecipe):
    """HQQ (DmxModule.hqq_quantizing): hp_gen maps the model to {module: DmxHQQHyperparams}; needs no calibration batch -- on exit every
    Linear / Conv2d among them has its weight replaced by ops.hqq_qdq of it, its `hqq_qparams` recorded and its weight cast's fake
    quantisation switched off"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.hqq_quantizing


class DmxAdaRoundRecipe(DmxBaseRecipe):
    """AdaRound (DmxModule.adaround_reconstructing): hp_gen maps the model to {module: DmxAdaRoundHyperparams}; the calibration
    forwards run inside the context, and on exit every Linear among them has its weight rounded element by element on its weight cast's
    own grid (ops.adaround_qdq) and its `adaround` record written"""

    def __init__(self, hp_gen, **kwargs):
        super().__init__(hp_gen, **kwargs)
        self.recipe_context_manager = DmxModule.adaround_reconstructing
