"""physdock_amd - MI355X-native sampler for PhysDock's redocking hot path.

    from physdock_amd import PhysDock, PhysDockConfig
    model = PhysDock(PhysDockConfig(model_name="medium")).to("cuda")
    model.load_state_dict(reference_state_dict)          # reference parameter names
    x = model.sample_diffusion(batch, num_sample=64, steps=40, karras_noise_schedule_power=1000)

Importing the package does not load the HIP library; the first kernel launch does, and
raises if `physdock_amd/libphysdock_hip.so` has not been built (python -m physdock_amd.build).
"""
from .configs import PhysDockConfig, small_config  # noqa: F401
from .import_weights import import_state_dict, import_unicore_ckpt  # noqa: F401
from .model import PhysDock, weighted_rigid_align  # noqa: F401
from .confidence import ConfidenceModule  # noqa: F401  (reference layers/confidence_module.py)
from .params import param_shapes, seeded_state_dict  # noqa: F401
from .driver import redock, redock_many  # noqa: F401  (multi-round caller of the sampler, reference redocking.py:156-342)
from .loss import PhysDockLoss  # noqa: F401  (reference models/loss.py:576-625, forward values; csrc/loss.hip)
from .loss import ConfidenceLoss, cal_lddt, pae_loss, pde_loss, plddt_loss  # noqa: F401  (reference models/loss.py:320-532; csrc/confidence_loss.hip)
from .metrics import (compute_plddt, compute_predicted_aligned_error, get_has_clash, get_metrics,  # noqa: F401
                      predicted_tm_score)  # (reference data/tools/get_metrics.py; csrc/metrics.hip)
from .symmetry import LigandSymmetry, automorphisms  # noqa: F401  (symmetry-corrected ligand RMSD for the ranking step; csrc/sym_rmsd.hip)
from .bestfit import BestFitRmsd  # noqa: F401  (superposed symmetry-corrected ligand RMSD: the conformer accuracy of a pose; csrc/bestfit_rmsd.hip)
from .bond_stereo import BondStereo  # noqa: F401  (cis / trans and twist of the stated double bonds of every pose; csrc/bond_stereo.hip)
from .torsions import TorsionFingerprint  # noqa: F401  (torsion angles and torsion-fingerprint deviation of ligand poses; csrc/torsion.hip)
from .validity import PoseValidity  # noqa: F401  (PoseBusters-style geometry checks of every pose; csrc/validity.hip)
from .lddt_pli import LddtPli  # noqa: F401  (symmetry-aware lDDT-PLI of every pose against the ground truth; csrc/lddt_pli.hip)
from .scoring import VinaScore  # noqa: F401  (Vina-style interaction score and forces of every pose; csrc/vina.hip)
from .interactions import InteractionFingerprint  # noqa: F401  (per-residue interaction fingerprint of every pose; csrc/plif.hip)
from .ring_interactions import RingInteractions  # noqa: F401  (pi-stacking, pi-cation and halogen bonds of every pose; csrc/plif_rings.hip)
from .hydrogens import Hydrogens  # noqa: F401  (riding hydrogens of every pose and angle-tested hydrogen bonds; csrc/hydrogens.hip)
from .receptor_geometry import ReceptorGeometry  # noqa: F401  (stereochemistry checks of every pose's receptor; csrc/receptor_geometry.hip)
from .pocket_accuracy import PocketAccuracy, swap_table_from_names  # noqa: F401  (lDDT-LP and pocket RMSD of every pose against the ground truth; csrc/pocket_accuracy.hip)
from .flex import FlexRefine, side_chain_torsions_from_names  # noqa: F401  (the same with flexible side chains; csrc/vina_flex.hip)
from .refine import VinaRefine  # noqa: F401  (rigid-body and torsion refinement of every pose in its receptor; csrc/vina_refine.hip)
from .pocket import PocketGrid  # noqa: F401  (pocket volume, enclosure and lining residues of every pose on a lattice; csrc/pocket.hip)
from .distogram import DistogramScore  # noqa: F401  (poses ranked by the trunk's own distogram, per-token detail, a potential with forces; csrc/distogram_score.hip)
from .surface import BuriedSurface  # noqa: F401  (ligand burial and interface area of every pose, Shrake - Rupley; csrc/sasa.hip)
from .clustering import PoseClusters  # noqa: F401  (binding modes of the poses: greedy leader clustering on the device; csrc/cluster.hip)
from .conformers import ConformerEnsemble  # noqa: F401  (distance-geometry conformers of a ligand, the template pool; csrc/conformers.hip)
from .sdfio import SdfTemplate, parse_sdf  # noqa: F401  (ligand poses as SD file records, formatted on the device, and their reader; csrc/sdf.hip)
from .smiles import parse_smiles  # noqa: F401  (a SMILES reader on the host, without a dependency)
from .ligand import Ligand, LigandLibrary  # noqa: F401  (ligands from SMILES to the reference's ligand feature blocks and a reference conformer; csrc/ligand_features.hip)
from .fingerprints import MorganFingerprint  # noqa: F401  (circular fingerprints of a ligand library, Tanimoto search and MaxMin picking; csrc/fingerprint.hip)
from .canonical import CanonicalForm, write_smiles  # noqa: F401  (canonical numbering, identity key and canonical SMILES of a ligand library; csrc/canonical.hip)
from .substructure import (SmartsPattern, SubstructureMatches, SubstructureQueries, parse_smarts,  # noqa: F401
                           pharmacophore_invariants)  # (SMARTS queries over a ligand library, matched atoms, pharmacophore classes; csrc/substructure.hip)
