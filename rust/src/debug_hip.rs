//! `hip` arm of `default_validate_constraints` (src/debug.rs:10-127): the body the reference leaves as a comment, with the
//! constraint evaluation on the device.  Every constraint is recorded with `Expr::graph_eval` into ONE register program (constraint k
//! ends in a STORE whose `b` is k), which `ms_validate_constraints` runs at every row of the trace domain under `Constraint::check`'s
//! semantics (src/constraints.rs:172-248) and answers, per constraint, with the first failing row and the number of failing rows.
//! `Div(a, b)` is `MUL(a, INV(b))` with `INV(0) = INV(None) = None`: every arm of `check`'s `Div` but `Div(None, 0)`, which the
//! reference maps to `Some(0)` and the device to `None` (the row is reported).  The report -- the unused-item warnings, then the
//! reference's message and panic for the lowest failing constraint -- is built on the host from the host-resident trace.
//! The same check in C++ and Python, tested against a checked model: ministark_amd/csrc/host/expr.hpp, ministark_amd/debug.py.
//!
//! Hook (src/debug.rs, first line of `default_validate_constraints`):
//!     #[cfg(feature = "hip")] return crate::debug_hip::validate_constraints(&<S::AirConfig as AirConfig>::constraints(base_trace.num_rows()), challenges, hints, base_trace, extension_trace);
//!
//! Source only (no Rust toolchain in the build image).
#![cfg(feature = "hip")]

use crate::constraints::AlgebraicItem;
use crate::constraints::Constraint;
use crate::expression::Expr;
use crate::utils::FieldVariant;
use crate::Matrix;
use crate::StarkExtensionOf;
use alloc::format;
use alloc::rc::Rc;
use alloc::string::String;
use alloc::vec::Vec;
use ark_ff::FftField;
use ark_poly::EvaluationDomain;
use ark_poly::Radix2EvaluationDomain;
use core::cell::RefCell;
use core::ffi::c_void;
use core::ops::Add;
use core::ops::Div;
use core::ops::Mul;
use core::ops::Neg;
use ministark_gpu::hip::field_id;
use ministark_gpu::hip::get_planner;
use ministark_gpu::hip::sys;
use ministark_gpu::hip::DeviceVec;
use ministark_gpu::GpuFftField;
use num_traits::Pow;

// opcodes of the constraint program (include/ministark_hip.h, enum ms_eval_op)
const X_P: u32 = 0;
const CONST_P: u32 = 1;
const CONST_Q: u32 = 2;
const TRACE_P: u32 = 3;
const TRACE_Q: u32 = 4;
const NEG_P: u32 = 7;
const ADD_PP: u32 = 9;
const MUL_PP: u32 = 12;
const INV_P: u32 = 15;
const POW_P: u32 = 17;
const STORE_Q: u32 = 20;
const STORE_P: u32 = 21;

/// A recorded node; `store = Some(k)`: the STORE of constraint k (no destination).
struct Node {
    op: u32,
    a: Option<usize>,
    b: Option<usize>,
    q: bool,
    imm0: u32,
    imm1: i32,
    store: Option<u32>,
}

#[derive(Default)]
struct Builder {
    nodes: Vec<Node>,
    consts: Vec<u64>, // Montgomery limbs, as the elements lie in memory
}

impl Builder {
    fn emit(&mut self, op: u32, q: bool, a: Option<usize>, b: Option<usize>, imm0: u32, imm1: i32) -> usize {
        self.nodes.push(Node { op, a, b, q, imm0, imm1, store: None });
        self.nodes.len() - 1
    }

    fn constant<T: Copy>(&mut self, v: &T) -> u32 {
        let off = self.consts.len() as u32;
        let p = v as *const T as *const u64;
        for i in 0..core::mem::size_of::<T>() / 8 {
            self.consts.push(unsafe { *p.add(i) });
        }
        off
    }
}

#[derive(Clone)]
struct Val {
    b: Rc<RefCell<Builder>>,
    id: usize,
}

impl Val {
    fn is_q(&self) -> bool {
        self.b.borrow().nodes[self.id].q
    }

    fn binary(self, rhs: Self, base: u32) -> Self {
        let (qa, qb) = (self.is_q(), rhs.is_q());
        let id = match (qa, qb) {
            (false, false) => self.b.borrow_mut().emit(base, false, Some(self.id), Some(rhs.id), 0, 0),
            (true, true) => self.b.borrow_mut().emit(base + 1, true, Some(self.id), Some(rhs.id), 0, 0),
            (true, false) => self.b.borrow_mut().emit(base + 2, true, Some(self.id), Some(rhs.id), 0, 0),
            (false, true) => self.b.borrow_mut().emit(base + 2, true, Some(rhs.id), Some(self.id), 0, 0),
        };
        Self { b: self.b, id }
    }

    fn unary(self, op_p: u32, imm0: u32) -> Self {
        let q = self.is_q();
        let id = self.b.borrow_mut().emit(op_p + u32::from(q), q, Some(self.id), None, imm0, 0);
        Self { b: self.b, id }
    }
}

impl Add for Val {
    type Output = Self;
    fn add(self, rhs: Self) -> Self {
        self.binary(rhs, ADD_PP)
    }
}

impl Mul for Val {
    type Output = Self;
    fn mul(self, rhs: Self) -> Self {
        self.binary(rhs, MUL_PP)
    }
}

impl Neg for Val {
    type Output = Self;
    fn neg(self) -> Self {
        self.unary(NEG_P, 0)
    }
}

impl Div for Val {
    type Output = Self;
    fn div(self, rhs: Self) -> Self {
        let inv = rhs.unary(INV_P, 0);
        self.binary(inv, MUL_PP)
    }
}

impl Pow<usize> for Val {
    type Output = Self;
    fn pow(self, exp: usize) -> Self {
        self.unary(POW_P, u32::try_from(exp).expect("exponent exceeds 32 bits"))
    }
}

/// Registers by a linear scan over the nodes; a STORE takes no register and frees its operand when that dies there.
fn assign_registers(nodes: &[Node]) -> Vec<u32> {
    let n = nodes.len();
    let mut last_use = alloc::vec![usize::MAX; n];
    for (k, node) in nodes.iter().enumerate() {
        for opnd in [node.a, node.b].into_iter().flatten() {
            last_use[opnd] = k;
        }
    }
    let (mut free_p, mut free_q) = (Vec::<u32>::new(), Vec::<u32>::new());
    let (mut next_p, mut next_q) = (0u32, 0u32);
    let mut reg = alloc::vec![0u32; n];
    let mut words = Vec::with_capacity(4 * n);
    for (k, node) in nodes.iter().enumerate() {
        let (a, b) = (node.a, if node.b == node.a { None } else { node.b });
        for opnd in [a, b].into_iter().flatten() {
            if last_use[opnd] == k {
                if nodes[opnd].q { free_q.push(reg[opnd]) } else { free_p.push(reg[opnd]) }
            }
        }
        if let Some(index) = node.store {
            words.extend_from_slice(&[node.op, 0, reg[node.a.unwrap()], index]);
            continue;
        }
        let r = if node.q {
            free_q.pop().unwrap_or_else(|| { next_q += 1; next_q - 1 })
        } else {
            free_p.pop().unwrap_or_else(|| { next_p += 1; next_p - 1 })
        };
        reg[k] = r;
        let (wa, wb) = match node.op {
            X_P => (0, 0),
            CONST_P | CONST_Q => (node.imm0, 0),
            TRACE_P | TRACE_Q => (node.imm0, node.imm1 as u32),
            op if op == POW_P || op == POW_P + 1 => (reg[node.a.unwrap()], node.imm0),
            _ => (reg[node.a.unwrap()], node.b.map_or(0, |b| reg[b])),
        };
        words.extend_from_slice(&[node.op, r, wa, wb]);
        if last_use[k] == usize::MAX {
            if node.q { free_q.push(r) } else { free_p.push(r) }
        }
    }
    assert!(next_p <= 256 && next_q <= 128, "constraint program needs too many registers (limits 256 Fp / 128 Fq)");
    words
}

pub fn validate_constraints<Fp: GpuFftField<FftField = Fp> + FftField, Fq: StarkExtensionOf<Fp>>(
    constraints: &[Constraint<FieldVariant<Fp, Fq>>],
    challenges: &[Fq],
    hints: &[Fq],
    base_trace: &Matrix<Fp>,
    extension_trace: Option<&Matrix<Fq>>,
) {
    use AlgebraicItem::*;
    use Expr::*;
    let n = base_trace.num_rows();
    let fq_is_ext = core::mem::size_of::<Fq>() != core::mem::size_of::<Fp>();
    let num_base = base_trace.num_cols();
    let num_ext = extension_trace.map_or(0, Matrix::num_cols);

    // ---- the reference's warnings
    let mut col_used = alloc::vec![false; num_base + num_ext];
    let mut challenge_used = alloc::vec![false; challenges.len()];
    let mut hint_used = alloc::vec![false; hints.len()];
    for constraint in constraints {
        constraint.traverse(&mut |node| match node {
            Leaf(Challenge(i)) => challenge_used[*i] = true,
            Leaf(Trace(i, _)) => col_used[*i] = true,
            Leaf(Hint(i)) => hint_used[*i] = true,
            _ => {}
        });
    }
    for (i, used) in col_used.iter().enumerate() { if !used { println!("WARN: no constraints for execution trace column {i}") } }
    for (i, used) in challenge_used.iter().enumerate() { if !used { println!("WARN: challenge at index {i} never used") } }
    for (i, used) in hint_used.iter().enumerate() { if !used { println!("WARN: hint at index {i} never used") } }

    // ---- every constraint into one program (periodic columns: not supported by this arm)
    let builder = Rc::new(RefCell::new(Builder::default()));
    let leaf = |op: u32, q: bool, imm0: u32, imm1: i32| {
        let id = builder.borrow_mut().emit(op, q, None, None, imm0, imm1);
        Val { b: Rc::clone(&builder), id }
    };
    let fq_const = |v: &Fq| {
        let off = builder.borrow_mut().constant(v);
        leaf(if fq_is_ext { CONST_Q } else { CONST_P }, fq_is_ext, off, 0)
    };
    for (k, constraint) in constraints.iter().enumerate() {
        let root = constraint.graph_eval(&mut |item| match *item {
            X => leaf(X_P, false, 0, 0),
            Constant(FieldVariant::Fp(v)) => {
                let off = builder.borrow_mut().constant(&v);
                leaf(CONST_P, false, off, 0)
            }
            Constant(FieldVariant::Fq(v)) => fq_const(&v),
            Challenge(i) => fq_const(&challenges[i]),
            Hint(i) => fq_const(&hints[i]),
            Trace(col, offset) => {
                let offset = i32::try_from(offset).unwrap();
                if col < num_base {
                    leaf(TRACE_P, false, col as u32, offset)
                } else {
                    leaf(if fq_is_ext { TRACE_Q } else { TRACE_P }, fq_is_ext, (col - num_base) as u32, offset)
                }
            }
            Periodic(_) => unimplemented!("periodic columns in the hip arm of validate_constraints"),
        });
        let q = root.is_q();
        let mut b = builder.borrow_mut();
        let st = b.emit(if q { STORE_Q } else { STORE_P }, q, Some(root.id), None, 0, 0);
        b.nodes[st].store = Some(k as u32);
    }
    let builder = Rc::try_unwrap(builder).ok().expect("no value outlives the walk").into_inner();
    let program = assign_registers(&builder.nodes);

    // ---- the trace to the device, one call
    let base_dev: Vec<DeviceVec<Fp>> = base_trace.0.iter().map(|c| DeviceVec::from_slice(c)).collect();
    let ext_dev: Vec<DeviceVec<Fq>> = extension_trace.map_or(Vec::new(), |m| m.0.iter().map(|c| DeviceVec::from_slice(c)).collect());
    let base_ptrs: Vec<*const c_void> = base_dev.iter().map(|c| c.device_ptr() as *const c_void).collect();
    let ext_ptrs: Vec<*const c_void> = ext_dev.iter().map(|c| c.device_ptr() as *const c_void).collect();
    let mut first_row = alloc::vec![u64::MAX; constraints.len()];
    let mut rows_failed = alloc::vec![0u64; constraints.len()];
    sys::check(unsafe {
        sys::ms_validate_constraints(
            get_planner().ctx(),
            field_id::<Fp>(),
            program.as_ptr(),
            (program.len() / 4) as u32,
            builder.consts.as_ptr() as *const c_void,
            builder.consts.len() as u32,
            n.trailing_zeros(),
            base_ptrs.as_ptr(),
            base_ptrs.len() as u32,
            ext_ptrs.as_ptr(),
            ext_ptrs.len() as u32,
            core::ptr::null(),
            core::ptr::null(),
            0,
            constraints.len() as u32,
            first_row.as_mut_ptr(),
            rows_failed.as_mut_ptr(),
        )
    });

    // ---- the lowest failing constraint: the reference's report and panic (src/debug.rs:97-121)
    for (c, (&f, &k)) in first_row.iter().zip(&rows_failed).enumerate() {
        if f != u64::MAX { println!("constraint {c}: fails at {k} rows, the first is row {f}") }
    }
    let Some(c_idx) = first_row.iter().position(|&r| r != u64::MAX) else { return };
    let row = first_row[c_idx] as usize;
    let trace_domain = Radix2EvaluationDomain::<Fp>::new(n).unwrap();
    let x = trace_domain.element(row);
    let get_trace_value = |col: usize, offset: isize| -> FieldVariant<Fp, Fq> {
        let pos = (row as isize + offset).rem_euclid(n as isize) as usize;
        if col < num_base {
            FieldVariant::Fp(base_trace.0[col][pos])
        } else {
            FieldVariant::Fq(extension_trace.unwrap().0[col - num_base][pos])
        }
    };
    let mut vals: Vec<String> = alloc::vec![format!("x = {x}")];
    constraints[c_idx].traverse(&mut |node| match *node {
        Leaf(Trace(col, offset)) => vals.push(format!("Trace(col={col:0>3}, offset={offset:0>3}) = {}", get_trace_value(col, offset))),
        Leaf(Challenge(i)) => vals.push(format!("Challenge({i}) = {}", challenges[i])),
        Leaf(Hint(i)) => vals.push(format!("Hint({i}) = {}", hints[i])),
        _ => (),
    });
    vals.sort();
    vals.dedup();
    eprint!("Constraint {c_idx} does not evaluate to a low degree polynomial. ");
    eprintln!("Divide by zero occurs at row {row}.\n");
    eprintln!("Expression values:\n{}", vals.join("\n"));
    panic!();
}
