'use strict'
// Non-integer numbers through the extension (the `floats` option, YGM_F_FLOATS): node test/floats.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs, with and without the option: what the extension
//          asks of the engine and what it does with a refusal
//  --gpu : the same through the N-API addon opened with { floats: true } (and one opened without), string for string
//          against yjs, and the addon against the committed fixtures (tests/golden/floats_v135.json.gz,
//          tests/golden/dtoa_v8.json.gz)
// A whiteboard document (shapes with x: 103.5, y: 40.25, an opacity, a 2^60 id) and a Tiptap document (lineHeight 1.5, a
// { pt: 10.5 } mark): with the option sharedJsonOf / jsonOf / versionSharedJson equal JSON.stringify on yjs's own
// document; without it the documents are left out and named ENONCANON, as before.
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const ROOT = path.join(__dirname, '..', '..', '..')
const Y = require(path.join(ROOT, 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle
const TJ = require(path.join(ROOT, 'tools', 'tojson_corpus.js'))      // the committed expectations over yjs's own document
const PJ = require(path.join(ROOT, 'tools', 'json_corpus.js'))
const CODES = { 1: 'EMALFORMED', 3: 'ENONCANON', 9: 'EUNSUPPORTED' }

const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const refused = st => Object.assign(new Error('refused'), { code: CODES[st] })

// test double (never shipped): the engine calls the extension makes, from yjs, with the refusal table of its `floats`
class Double {
  constructor (floats) { this.floats = !!floats; this.log = [] }
  _table () { TJ.setFloats(this.floats); PJ.setFloats(this.floats) }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) { return states.map((s, i) => yjsRestore(s, versions[i], !(opts && isNoGc(opts[i])))) }
  async toJsonMany (states, names, kind) {
    this.log.push(['toJsonMany', states.length, kind])
    this._table()
    try { return states.map((s, i) => { const r = TJ.ask(s, String(names[i]), kind); return r[2] === 0 ? r[3] : refused(r[2]) }) } finally { TJ.setFloats(false); PJ.setFloats(false) }
  }
  async jsonMany (states, names) {
    this.log.push(['jsonMany', states.length])
    this._table()
    try { return states.map((s, i) => { const r = PJ.rootsOf(s).find(q => q[0] === Buffer.from(String(names[i])).toString('hex')); return r[1] === 0 ? r[2] : refused(r[1]) }) } finally { TJ.setFloats(false); PJ.setFloats(false) }
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine (floats) {
  if (mode === 'cpu') return new Double(floats)
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true, floats })
}

function shape (shapes, id, x, y) {
  const s = new Y.Map()
  shapes.set(id, s)
  s.set('x', x); s.set('y', y); s.set('opacity', 0.35); s.set('scale', 1 / 3); s.set('big', 1152921504606846976); s.set('tiny', 1.5e-7)
  s.set('points', [[0.5, 1.25], [103.5, 40.25], [1e21, -2.5]])
  return s
}
function tiptap (doc) {
  const p = new Y.XmlElement('paragraph')
  doc.getXmlFragment('default').insert(0, [p])
  p.setAttribute('lineHeight', 1.5); p.setAttribute('width', 0.5)
  const t = new Y.XmlText()
  p.insert(0, [t])
  t.insert(0, 'sized', { size: { pt: 10.5 } })
}

for (const floats of [true, false]) {
  test_('a whiteboard and a Tiptap document with floats: ' + floats, async () => {
    const engine = makeEngine(floats)
    const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
    try {
      const x = await openDoc(ext, 'board', false, 51)
      const d = await openDoc(ext, 'page', false, 52)
      const shapes = x.document.getMap('shapes')
      shape(shapes, 's1', 103.5, 40.25)
      tiptap(d.document)
      const v0 = (await ext.takeVersions(['board'])).get('board')
      const at0 = JSON.stringify(shapes.toJSON())
      shape(shapes, 's2', -0.000001, 123456.789)
      const now = JSON.stringify(shapes.toJSON())
      assert.ok(now.includes('"x":103.5,"y":40.25,"opacity":0.35,"scale":0.3333333333333333,"big":1152921504606847000,"tiny":1.5e-7,"points":[[0.5,1.25],[103.5,40.25],[1e+21,-2.5]]'), now)

      const got = await ext.sharedJsonOf(['board'], { root: 'shapes' })
      const page = await ext.jsonOf(['page'])
      const res = await ext.versionSharedJson([{ documentName: 'board', version: v0 }], { root: 'shapes' })
      if (floats) {
        assert.strictEqual(got.get('board'), now)
        assert.strictEqual(page.get('page'), '{"type":"doc","content":[{"type":"paragraph","attrs":{"lineHeight":1.5,"width":0.5},"content":[{"type":"text","text":"sized","marks":[{"type":"size","attrs":{"pt":10.5}}]}]}]}')
        assert.strictEqual(res[0].value, at0)
        assert.deepStrictEqual(ext.unserialized, [])
      } else {   // without the option nothing moves: left out and named, the caller keeps its yjs path
        assert.deepStrictEqual([Array.from(got.keys()), Array.from(page.keys()), res[0].status], [[], [], 'rejected'])
        assert.deepStrictEqual(ext.unserialized.map(u => [u.documentName, u.code]), [['board', 'ENONCANON'], ['page', 'ENONCANON'], ['board', 'ENONCANON']])
      }
      if (mode === 'cpu') assert.deepStrictEqual(engine.log, [['toJsonMany', 1, 0], ['jsonMany', 1], ['toJsonMany', 1, 0]])
    } finally { engine.close() }
  })
}

test_('GpuEngine and GpuMerge pass the option on as flag 8', async () => {
  assert.ok(/this\.flags = \(opts\.compat135 \? 1 : 0\) \| \(opts\.floats \? 8 : 0\)/.test(fs.readFileSync(path.join(__dirname, '..', 'src', 'engine.js'), 'utf8')))
  assert.ok(/floats: c\.floats/.test(fs.readFileSync(path.join(__dirname, '..', 'src', 'index.js'), 'utf8')))
  if (mode === 'gpu') {
    const { GpuEngine } = require('../src/engine.js')
    const e = new GpuMerge({ floats: true, device: 0, store: new MemoryStore(), Y })._engine()
    try { assert.strictEqual(e.flags & 8, 8) } finally { e.close() }
    const plain = new GpuEngine({ device: 0 })
    try { assert.strictEqual(plain.flags & 8, 0) } finally { plain.close() }
  }
})

if (mode === 'gpu') {
  test_('the addon against floats_v135 and dtoa_v8: strings in caller order, refusals alone; without the option status 3', async () => {
    const { GpuEngine } = require('../src/engine.js')
    const on = new GpuEngine({ device: 0, floats: true })
    const off = new GpuEngine({ device: 0 })
    try {
      const fix = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'floats_v135.json.gz'))).toString())
      let n = 0; let was3 = 0
      const check = (rows, got, gotOff) => rows.forEach((r, i) => {
        if (r.st === 0) assert.strictEqual(got[i], r.js, r.note)
        else assert.ok(got[i] instanceof Error && got[i].code === CODES[r.st], r.note + ': ' + String(got[i]))
        if (r.off === 0) assert.strictEqual(gotOff[i], r.js, r.note)
        else assert.ok(gotOff[i] instanceof Error && gotOff[i].code === CODES[r.off], r.note + ' (off): ' + String(gotOff[i]))
        n++; if (r.st === 0 && r.off === 3) was3++
      })
      for (const kind of [0, 1, 2]) {
        const rows = []
        for (const e of fix.tojson) for (const r of e.asks) if (r[1] === kind) rows.push({ note: e.note, state: Buffer.from(e.state, 'hex'), name: Buffer.from(r[0], 'hex'), st: r[2], js: Buffer.from(r[3], 'hex').toString('utf8'), off: r[4] })
        check(rows, await on.toJsonMany(rows.map(r => r.state), rows.map(r => r.name), kind), await off.toJsonMany(rows.map(r => r.state), rows.map(r => r.name), kind))
      }
      const pm = []
      for (const e of fix.json) for (const r of e.asks) pm.push({ note: e.note, state: Buffer.from(e.state, 'hex'), name: Buffer.from(r[0], 'hex'), st: r[1], js: Buffer.from(r[2], 'hex').toString('utf8'), off: r[3] })
      check(pm, await on.jsonMany(pm.map(r => r.state), pm.map(r => r.name)), await off.jsonMany(pm.map(r => r.state), pm.map(r => r.name)))
      const fl = []
      for (const e of fix.fields) for (const r of e.asks) fl.push({ note: e.note, state: Buffer.from(e.state, 'hex'), fields: r[0] === null ? null : r[0].map(h => Buffer.from(h, 'hex')), st: r[1], js: Buffer.from(r[2], 'hex').toString('utf8'), off: r[3] })
      check(fl, await on.jsonFieldsMany(fl.map(r => r.state), fl.map(r => r.fields)), await off.jsonFieldsMany(fl.map(r => r.state), fl.map(r => r.fields)))
      assert.ok(n >= 380 && was3 >= 180, n + ' ' + was3)
      // V8's own strings, through a live yjs document
      const v8 = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'dtoa_v8.json.gz'))).toString()).doubles
      const xs = v8.map(([h]) => Buffer.from(h, 'hex').readDoubleBE(0)).filter(x => !(Number.isInteger(x) && x < -2147483647)).slice(0, 1500)
      const d = new Y.Doc(); d.clientID = 61
      d.getArray('a').push(xs)
      assert.deepStrictEqual(await on.toJsonMany([Y.encodeStateAsUpdate(d)], ['a'], 1), [JSON.stringify(xs)])
    } finally { on.close(); off.close() }
  })
}

function test_ (name, fn) { (test_.all = test_.all || []).push({ name, fn }) }

;(async () => {
  let failed = 0
  for (const t of test_.all) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : test_.all.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
